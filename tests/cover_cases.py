"""Cases for the coverage walk (coverage_walk_body in csrc/gtx_kernels.hip, bucket_cover_kernel in csrc/gtx_bucket.hip) that sit on its
seams instead of in the interior of its paths: the 63-slot window edge, the third window exchange, the slot a step ends in, the
shifted second window against the sentinels, the spread limits of the 32-bit prefix sums, keys equal to thresholds, runs of equal
thresholds, histogram tile borders inside a flush, span edges and the cuts of the partition kernel.

Shared by tests/test_cover_cases_cpu.py (no GPU: the references against each other and against the oracle, every family's aim) and
tests/test_gpu_cover_seams.py.  brute() is the definition of the reduction, brute_py() the same in Python integers, thresholds() and
crossings() restate what the host builds (cover_prepare in csrc/gtx_capi.hip) so that every family can state what it aims at.
SRC pins the kernel constants the cases aim at: name -> (source file under csrc/, regular expression, the values of its groups);
a pattern may match several times (every give-up count), then every match carries the same values."""
import collections
import functools
import zlib

import numpy as np

READS_SORTED, READS_UNSORTED = 1, 16

KSLOTS = 63                     # slots per register window
STEP = 256                      # reads per step (4 x 64)
CHUNK = 64                      # reads per chunk
SPREAD_STEP = 1 << 22           # a step's keys spread less than this (32-bit prefix sums of 256 relative keys)
SPREAD_CHUNK = 1 << 24          # a chunk's keys spread less than this (64 relative keys)
GIVE_UP_FWD = 2                 # window exchanges a step or a chunk makes; one more and its lanes add themselves
GIVE_UP_BACK = 6                # slots the general walk steps back; one more and it seeks
MIN_CPW = 8                     # chunks per wave (the span), at least
TILE_SHIFT = 10
TILE = 1 << TILE_SHIFT          # histogram slots per tile; slot = rank + class id
BKT_E = 2048                    # thresholds per bucket of the partition path
BKT_T = 2560                    # thresholds of a bucket's slice in LDS
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
TOP = (1 << 31) - 2             # the largest coordinate of a read
REF_TOP = TOP - 1               # ... of a region: gtx_set_refs refuses 2^31 - 2

SRC = {
    "KSLOTS": ("gtx_kernels.hip", r"static constexpr int kSlots = (\d+);", (KSLOTS,)),
    "SPREAD_STEP": ("gtx_kernels.hip", r"if \(\(unsigned\)\(ktop - kbase\) >= \(1u << (\d+)\) \|\| WIN::below\(kbase, X\.prevW\)\) return false;",
                    (SPREAD_STEP.bit_length() - 1,)),
    "SPREAD_CHUNK": ("gtx_kernels.hip", r"const bool ok = valid && \(unsigned\)\(ktop - kbase\) < \(1u << (\d+)\) && ", (SPREAD_CHUNK.bit_length() - 1,)),
    "GIVE_UP_FWD": ("gtx_kernels.hip", r"\+\+adv > (\d+)", (GIVE_UP_FWD,)),
    "GIVE_UP_BACK": ("gtx_kernels.hip", r"\+\+nback > (\d+)", (GIVE_UP_BACK,)),
    "STEP": ("gtx_kernels.hip", r"&& at \+ (\d+) <= nMine && st\.sg\.cls >= 0\)", (STEP,)),
    "MIN_CPW": ("gtx_routes.h", r"\(int\)std::min<long long>\((\d+), std::max<long long>\((\d+), \(\(nReads \+ 63\) >> 6\) / (\d+)\)\);", (64, MIN_CPW, 24576)),
    "TILE_SHIFT": ("gtx_routes.h", r"constexpr int kTileShift = (\d+);", (TILE_SHIFT,)),
    "BKT_E": ("gtx_bucket.hip", r"static constexpr int kBktE = (\d+), kBktS = (\d+);", (BKT_E, 4096)),
    "BKT_T": ("gtx_bucket.hip", r"static constexpr int kBktT = (\d+), kCellsT = (\d+);", (BKT_T, 2560)),
    "BKT_CUT_RULE": ("gtx_capi.hip", r"k\.sLo\.push_back\(e0\); k\.sHi\.push_back\(\(int32_t\)std::min<int64_t>\(\(int64_t\)e0 \+ kS, s1\)\);", ()),
    "REF_TOP": ("gtx_capi.hip", r"if \(s >= INT32_MAX - (\d+) \|\| e >= INT32_MAX - (\d+)\) return fail\(c, GTX_E_RANGE, ", (INT32_MAX - REF_TOP - 1, INT32_MAX - REF_TOP - 1)),
    "PLACE_BUDGET": ("gtx_capi.hip", r"const int64_t budget = std::max<int64_t>\((\d+), nv / (\d+)\) \+ (\d+) \* \(int64_t\)nClasses;", (1024, 8, 2)),
    "PLACE_CELLS": ("gtx_capi.hip", r"return \(top >> sh\) \+ (\d+);", (2,)),
    "PLACE_IN_WINDOW": ("gtx_kernels.hip", r"if \(c0 == preCls && \(ms & 1\) && \(me & 1\) && \(i64\)ms >= 0 && \(i64\)me >= 0\) \{", ()),
    "SLOT_RULE": ("gtx_capi.hip", r"\? posTS : posTE\)\[k\] = \(int32_t\)\(i \+ it\[i\]\.cls\);", ()),
}
ROUTE_MIN_CPW = [("cover_cpw 1 0", str(MIN_CPW)), ("cover_cpw %d 0" % (MIN_CPW * CHUNK + 1), str(MIN_CPW)), ("cover_cpw 1 12", "12"), ("cover_cpw 1 16", "16")]

Case = collections.namedtuple("Case", "name refs n_classes reads weights flags")
VARIANTS = ("none", "small", "signed", "zero")
FAMILIES = "ABCDEFGI"            # (H streams the cases of A)


# ---- references ----------------------------------------------------------------------------------------------------------------
def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1, 3)


def taking_part(refs):
    """the regions that count under the library's rule"""
    r = _i64(refs)
    return (r[:, 0] >= 0) & ~((r[:, 1] > r[:, 2]) | (r[:, 2] <= 0))


def brute_multi(refs, reads, ws, block=256):
    """brute() for several weight vectors over one geometry (the overlap lengths are computed once)"""
    r, q = _i64(refs), _i64(reads)
    take, ok = taking_part(r), q[:, 1] <= q[:, 2]
    W = [(np.ones(len(q), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)).astype(np.uint64) for w in ws]
    out = [np.zeros(len(r), dtype=np.uint64) for _ in ws]
    qc, s, e = q[:, 0][None, :], q[:, 1][None, :], q[:, 2][None, :]
    for b in range(0, len(r), block):
        sl = slice(b, b + block)
        C, S, E = r[sl, 0][:, None], r[sl, 1][:, None], r[sl, 2][:, None]
        hit = take[sl, None] & ok[None, :] & (qc == C) & (s <= E) & (e >= S)
        ln = np.where(hit, np.minimum(e, E) - np.maximum(s, S) + 1, 0).astype(np.uint64)
        for o, w in zip(out, W):
            o[sl] = ln @ w                                         # uint64: exactly mod 2^64
    return out


def brute(refs, reads, w=None):
    """cov[k] = sum of w_q (min(e_q, E_k) - max(s_q, S_k) + 1) over the reads of k's class with s_q <= e_q that overlap k, mod 2^64"""
    return brute_multi(refs, reads, [w])[0]


def brute_py_multi(refs, reads, ws):
    """the same in Python integers, reduced mod 2^64 at the end; several weight vectors over one geometry"""
    r, q = _i64(refs).tolist(), _i64(reads).tolist()
    W = [[1] * len(q) if w is None else [int(x) for x in w] for w in ws]
    by_class = {}
    for i, (qc, s, e) in enumerate(q):
        if s <= e:
            by_class.setdefault(qc, []).append((i, s, e))
    out = [[] for _ in ws]
    for c, S, E in r:
        hits = []
        if c >= 0 and not (S > E or E <= 0):
            hits = [(i, min(e, E) - max(s, S) + 1) for i, s, e in by_class.get(c, ()) if s <= E and e >= S]
        for o, w in zip(out, W):
            o.append(sum(w[i] * ln for i, ln in hits) % (1 << 64))
    return [np.array(o, dtype=np.uint64) for o in out]


def brute_py(refs, reads, w=None):
    return brute_py_multi(refs, reads, [w])[0]


def thresholds(refs, n_classes):
    """what cover_prepare builds: E_k and S_k - 1 of the regions that take part, sorted per class; (T, seg), class c = T[seg[c]:seg[c+1]]"""
    r = _i64(refs)[taking_part(refs)]
    cls = np.concatenate([r[:, 0], r[:, 0]])
    val = np.concatenate([r[:, 2], r[:, 1] - 1])
    o = np.lexsort((val, cls))
    seg = np.zeros(n_classes + 1, dtype=np.int64)
    np.add.at(seg, cls + 1, 1)
    return val[o], np.cumsum(seg)


def rank(T, x):
    """#{T < x}: the slot of key x"""
    return np.searchsorted(T, x, side="left")


def class_thresholds(refs, n_classes, c):
    T, seg = thresholds(refs, n_classes)
    return T[seg[c]:seg[c + 1]]


def crossings(refs, reads, at, n, n_classes=None):
    """thresholds between the first and the last key of the reads [at, at + n) of one class: (for the starts, for the ends)"""
    q = _i64(reads)[at:at + n]
    assert len(q) == n and (q[:, 0] == q[0, 0]).all()
    nc = int(max(_i64(refs)[:, 0].max(), q[0, 0]) + 1) if n_classes is None else n_classes
    T = class_thresholds(refs, nc, int(q[0, 0]))
    return tuple(int(rank(T, q[-1, k]) - rank(T, q[0, k])) for k in (1, 2))


def place_table(refs, n_classes):
    """make_place_table of csrc/gtx_capi.hip over the thresholds: (shift, T, seg, cells per class); a cell is 2^shift positions and
    stands for the thresholds of its class below its first position (cell 0: none)"""
    T, seg = thresholds(refs, n_classes)
    budget = max(1024, len(T) // 8) + 2 * n_classes

    def cells(c, sh):
        return 0 if seg[c] == seg[c + 1] else (max(0, int(T[seg[c + 1] - 1])) >> sh) + 2
    sh = 0
    while sum(cells(c, sh) for c in range(n_classes)) > budget and sh < 31:
        sh += 1
    return sh, T, seg, [cells(c, sh) for c in range(n_classes)]


def table_rank(pt, c, key):
    """the rank (within class c) the place table holds for the cell of `key`"""
    sh, T, seg, nc = pt
    cell = min(max(int(key), 0) >> sh, nc[c] - 1)
    return 0 if cell == 0 else int(rank(T[seg[c]:seg[c + 1]], cell << sh))


def class_rank(pt, c, key):
    return int(rank(pt[1][pt[2][c]:pt[2][c + 1]], key))


def placed(pt, c, table_key, kmin):
    """where a window of class c stands after a placement through the table: (rank of its slot 0 within the class, slot) -- the window
    loaded at the rank of table_key's cell if the smallest key kmin falls into its 63 slots, else slot 0 at kmin's own rank"""
    pre, r = table_rank(pt, c, table_key), class_rank(pt, c, kmin)
    return (pre, r - pre) if 0 <= r - pre < KSLOTS else (r, 0)


def head_of_span(pt, reads, at, n=STEP):
    """both windows at the head of a span whose first step is the reads [at, at + n) of one class: ((base, slot) for the starts, for the
    ends); the table is asked for the first read's start, and unless BOTH smallest keys fall into that window both are placed exactly"""
    q = _i64(reads)[at:at + n]
    c, pre = int(q[0, 0]), table_rank(pt, int(q[0, 0]), q[0, 1])
    ranks = [class_rank(pt, c, q[:, k].min()) for k in (1, 2)]
    if all(0 <= r - pre < KSLOTS for r in ranks):
        return tuple((pre, r - pre) for r in ranks)
    return tuple((r, 0) for r in ranks)


def after_keys(pt, c, win, last_key):
    """the window (base, slot) after ordered keys up to last_key went through it: it slides by 63 slots while the key lies beyond it
    (at most GIVE_UP_FWD times, else the step or chunk gives up and the model ends)"""
    r = class_rank(pt, c, last_key)
    base, n = win[0], 0
    while r > base + KSLOTS - 1:
        base, n = base + KSLOTS, n + 1
    assert n <= GIVE_UP_FWD, "the model does not follow a give-up"
    return base, r - base


def expected_info(case):
    """n_no_class, n_degenerate (inverted reads of a known class; zero-length ones are dropped silently), first_degenerate"""
    q = _i64(case.reads)
    noclass = (q[:, 0] < 0) | (q[:, 0] >= case.n_classes)
    inv = ~noclass & (q[:, 1] > q[:, 2] + 1)
    return {"n_no_class": int(noclass.sum()), "n_degenerate": int(inv.sum()), "first_degenerate": int(np.flatnonzero(inv)[0]) if inv.any() else None}


def oracle_takes(case):
    """the reads the oracle returns a result for: it refuses s > e and e <= 0, and knows no class outside 0 .. n_classes - 1"""
    q = _i64(case.reads)
    return (q[:, 0] >= 0) & (q[:, 0] < case.n_classes) & (q[:, 1] <= q[:, 2]) & (q[:, 2] > 0)


def weights_for(name, n, variant):
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (name, variant)).encode()))
    if variant == "none":
        return None
    if variant == "small":
        return rng.integers(0, 10, size=n).astype(np.int32)
    if variant == "zero":
        return np.zeros(n, dtype=np.int32)
    w = rng.integers(INT32_MIN, INT32_MAX + 1, size=n).astype(np.int32)
    ext = rng.integers(0, n, size=max(2, n // 16))
    w[ext[::2]] = INT32_MIN
    w[ext[1::2]] = INT32_MAX
    w[0] = INT32_MIN
    w[-1] = INT32_MAX if n > 1 else INT32_MIN
    return w


# ---- builders ------------------------------------------------------------------------------------------------------------------
def tri(c, s, e):
    s = np.asarray(s, dtype=np.int64)
    out = np.empty((len(s), 3), dtype=np.int64)
    out[:, 0], out[:, 1], out[:, 2] = c, s, e
    assert out[:, 1:].min() >= INT32_MIN and out[:, 1:].max() <= INT32_MAX
    return out.astype(np.int32)


def regions_of(ts, cls=0, far=None):
    """regions of class cls whose thresholds are exactly the distinct values ts (and `far`, above them, when they are odd in number):
    consecutive thresholds t < u make the region [t + 1, u]"""
    ts = np.unique(np.asarray(ts, dtype=np.int64))
    if len(ts) == 0:
        ts = np.array([far - 10], dtype=np.int64)                          # (no threshold asked for: one region above everything)
    if len(ts) % 2:
        assert far is not None and far > ts[-1]
        ts = np.append(ts, far)
    return tri(cls, ts[0::2] + 1, ts[1::2])


def regions_split(ts, cls=0):
    """the same for sorted values that may repeat: threshold i pairs with threshold i + n/2"""
    ts = np.sort(np.asarray(ts, dtype=np.int64))
    h = len(ts) // 2
    assert len(ts) == 2 * h and (ts[:h] < ts[h:]).all()
    return tri(cls, ts[:h] + 1, ts[h:])


def spread(lo, hi, c):
    """c distinct integers of [lo, hi), evenly spread"""
    assert 0 <= c <= hi - lo, (lo, hi, c)
    return (lo + np.unique(np.linspace(0, hi - lo - 1, c).astype(np.int64))) if c else np.zeros(0, dtype=np.int64)


def both_cross(reads, at, n):
    """the values T with first <= T < last for the starts AND for the ends of the reads [at, at + n): crossed by both windows"""
    q = _i64(reads)
    return int(max(q[at, 1], q[at, 2])), int(min(q[at + n - 1, 1], q[at + n - 1, 2]))


# ---- A: sizes and spans --------------------------------------------------------------------------------------------------------
A_SIZES = (1, 63, 64, 65, 255, 256, 257, 319, 320, 511, 512, 513, 575, 767, 768, 769, 1023, 1024, 1025, 1537)
A_CPW = (MIN_CPW, 12, 16)


def family_a():
    for n in A_SIZES:
        s = 1000 + 10 * np.arange(n)
        S = 1003 + 80 * np.arange(max(1, n // 8))
        yield Case("A-n%d" % n, tri(0, S, S + 50), 1, tri(0, s, s + 35), None, READS_SORTED)
    for edge in (STEP,) + tuple(cpw * CHUNK for cpw in A_CPW):          # no step / one step; each span's last read, and the next wave's first
        assert {edge - 1, edge, edge + 1} <= set(A_SIZES)
    for cpw in A_CPW:                                                   # the second wave's head placement with fewer and with more than a step
        assert any(0 < n - cpw * CHUNK < STEP for n in A_SIZES) and any(n - cpw * CHUNK >= STEP for n in A_SIZES)
    assert {STEP + CHUNK - 1, STEP + CHUNK} <= set(A_SIZES)             # a step and a partial / a full chunk


# ---- B: boundaries crossed by one step -----------------------------------------------------------------------------------------
B_P = (0, 1, 31, 62, 63)
B_C = (0, 1, 2, 62, 63, 64, 125, 126, 127, 188, 189, 190, 191, 252, 253, 400, 1000)
B_KINDS = ("eq", "uneq", "bp1")
B_POS = (0, 1, 3)                                                       # first, second, last in a span of four (16 chunks per wave)
B_GAP, B_BASE, B_STEPS = 8, 20031, 5                                    # (the first key is the last position of a 64-position cell)


def b_case(p, c, kind, pos):
    n = B_STEPS * STEP
    i = np.arange(n)
    s = B_BASE + B_GAP * i
    e = s + {"eq": 2, "uneq": 2 + i % 3, "bp1": 0}[kind]
    reads = tri(0, s, e)
    # the lead-in moves the slot the windows stand in when the swept step begins.  First in its span: p thresholds right below the first
    # key, inside its cell of the place table (the head placement loads the window at the cell's rank and stands in slot p).  Later in the
    # span: the step before crosses p thresholds, the ones before that none (slot 0 at the head, slot p after them).  The steps behind the
    # swept one are plain: three thresholds each.
    ts = [B_BASE - 1 - np.arange(p if pos == 0 else 0)]
    for k in range(B_STEPS):
        lo, hi = both_cross(reads, k * STEP, STEP)
        ts.append(spread(lo, hi, c if k == pos else p if k == pos - 1 else 0 if k < pos else 3))
    far = int(e[-1]) + 5000
    ts.append(np.array([far - 20, far - 10]))                           # (one region above everything: the place table's cells stay 64 positions)
    refs = regions_of(np.concatenate(ts), far=far)
    return Case("B-p%d-c%d-%s-pos%d" % (p, c, kind, pos), refs, 1, reads, None, READS_SORTED)


def family_b():
    seen_s, seen_e, slots = set(), set(), {(pos, k): set() for pos in B_POS for k in (0, 1)}
    for kind in B_KINDS:
        for pos in B_POS:
            for p in B_P:
                for c in B_C:
                    case = b_case(p, c, kind, pos)
                    cs, ce = crossings(case.refs, case.reads, pos * STEP, STEP)
                    assert cs == c and ce == c, case.name
                    for k in range(pos + 1, B_STEPS):
                        assert crossings(case.refs, case.reads, k * STEP, STEP) == (3, 3), case.name
                    seen_s.add(cs), seen_e.add(ce)
                    # the slot each window stands in when the swept step begins, with 16 chunks per wave (the span is the steps 0 .. 3):
                    # the head placement restated, then the steps before the swept one
                    pt = place_table(case.refs, 1)
                    wins = head_of_span(pt, case.reads, 0)
                    for k in (0, 1):
                        w = wins[k]
                        for st in range(pos):
                            w = after_keys(pt, 0, w, case.reads[st * STEP + STEP - 1, 1 + k])
                        assert w[1] == p % KSLOTS and w[0] + w[1] == rank(pt[1], case.reads[pos * STEP, 1 + k]), case.name
                        slots[(pos, k)].add(w[1])
                    yield case
    assert seen_s == set(B_C) and seen_e == set(B_C)
    for got in slots.values():                                          # the swept step begins in the first, the second, a middle and the last slot of
        assert got == {0, 1, 31, KSLOTS - 1}                            # a window (p = 63: the window was exchanged, or placed anew, slot 0), both windows
    # one, two, three windows and the give-up: a window takes 63 slots, a step gives up after the third exchange
    assert {KSLOTS - 1, KSLOTS, KSLOTS + 1, 3 * KSLOTS - 1, 3 * KSLOTS, 3 * KSLOTS + 1, 4 * KSLOTS, 4 * KSLOTS + 1} <= set(B_C)


# ---- C: the same crossings without a step --------------------------------------------------------------------------------------
C_SIZES = (64, 128, 192, 65, 100)
C_GAP, C_BASE = 17, 30015                                               # (the last position of a 64-position cell)
C_DESCENTS = (1, 5, 6, 7, 8, 63, 64, 200)
C_LANES = (1, 32, 63)


def c_case(n, c, p):
    s = C_BASE + C_GAP * np.arange(n)
    reads = tri(0, s, s + 2)
    ts = [C_BASE - 1 - np.arange(p)]                                    # inside the first key's cell: the windows stand in slot p
    for at in range(0, n, CHUNK):
        cnt = min(CHUNK, n - at)
        lo, hi = both_cross(reads, at, cnt)
        if hi > lo:
            ts.append(spread(lo, hi, min(c, hi - lo)))
    far = int(s[-1]) + 5000
    ts.append(np.array([far - 20, far - 10]))                           # (one region above everything: the place table's cells stay 64 positions)
    return Case("C-n%d-c%d-p%d" % (n, c, p), regions_of(np.concatenate(ts), far=far), 1, reads, None, READS_SORTED)


C_LEFT_IN = (0, 2, 5, 6, 30, 62)                                        # the slot the chunk before the descent leaves the starts' window in


def c_descent(n, b, lane, o):
    """a threshold at every position (and one region above everything: the place table's cells are 64 positions, a window loaded through
    it stands in any of its slots); key i has rank 300 + o + i, but the key at `lane` of the LAST chunk lies b slots below the slot the
    chunk before it left the windows in (the rank of that chunk's last key): the general walk steps back b slots, or seeks"""
    T = np.concatenate([C_BASE + np.arange(640), [C_BASE + 5640, C_BASE + 5650]])
    r = 300 + o + np.arange(n)
    at = n - CHUNK
    r[at + lane] = r[at - 1] - b
    s = C_BASE + r
    return Case("C-descent-n%d-b%d-lane%d-o%d" % (n, b, lane, o), regions_of(T), 1, tri(0, s, s + 2), None, READS_SORTED)


def c_left(case, k):
    """the window (base, slot) of the starts (k = 0) or the ends (k = 1) when the last chunk of a chunk-only case begins"""
    pt = place_table(case.refs, 1)
    q = _i64(case.reads)
    w = placed(pt, 0, q[:CHUNK, 1].min(), q[:CHUNK, 1 + k].min())
    for at in range(0, len(q) - CHUNK, CHUNK):
        w = after_keys(pt, 0, w, q[at + CHUNK - 1, 1 + k])
    return w


@functools.lru_cache(maxsize=None)
def c_offsets(n):
    """for each slot of C_LEFT_IN an offset o of the keys' ranks that leaves the starts' window there"""
    found = {}
    for o in range(2 * KSLOTS):
        found.setdefault(c_left(c_descent(n, 1, 1, o), 0)[1], o)
    assert set(C_LEFT_IN) <= set(found)
    return tuple(found[j] for j in C_LEFT_IN)


def family_c():
    seen = set()
    for n in C_SIZES:
        for p in (0, 62):
            for c in B_C:
                case = c_case(n, c, p)
                pt = place_table(case.refs, 1)
                assert placed(pt, 0, case.reads[0, 1], case.reads[0, 1])[1] == p and placed(pt, 0, case.reads[0, 1], case.reads[0, 2])[1] == p
                for at in range(0, n - CHUNK + 1, CHUNK):
                    assert crossings(case.refs, case.reads, at, CHUNK) == (c, c), case.name
                    seen.add(c)
                yield case
    assert seen == set(B_C) and all(n < STEP for n in C_SIZES)
    back_over_the_edge = set()
    for n in (2 * CHUNK, 3 * CHUNK):
        for b in C_DESCENTS:
            for lane in C_LANES:
                for o, left_in in zip(c_offsets(n), C_LEFT_IN):
                    case = c_descent(n, b, lane, o)
                    T = class_thresholds(case.refs, 1, 0)
                    for k in (0, 1):                                     # both windows stand b slots above the key when its chunk begins
                        base, j = c_left(case, k)
                        assert base + j - rank(T, case.reads[n - CHUNK + lane, 1 + k]) == b, case.name
                        assert rank(T, case.reads[n - CHUNK:, 1 + k]).min() == base + j - b
                        if b <= GIVE_UP_BACK and j < b:
                            back_over_the_edge.add((k, b))
                    assert c_left(case, 0)[1] == left_in
                    yield case
    # six slots back without a seek and seven with one; stepping back over the lower edge of a window (the exchange in back()); whole windows back
    assert {GIVE_UP_BACK, GIVE_UP_BACK + 1, KSLOTS, KSLOTS + 1} <= set(C_DESCENTS)
    assert {(k, b) for k in (0, 1) for b in (5, GIVE_UP_BACK)} <= back_over_the_edge


# ---- D: equal keys and thresholds ----------------------------------------------------------------------------------------------
D_RUNS = (2, 62, 63, 64, 126, 189, 190, 300)


def d_runs(r):
    """r regions with one E (1000), r with one S (2000): runs of r equal thresholds at 1000 and at 1999"""
    i = np.arange(r)
    return np.concatenate([tri(0, 100 + i, np.full(r, 1000)), tri(0, np.full(r, 2000), 2100 + i)])


def family_d():
    refs = np.array([[0, 100, 200], [0, 201, 300], [0, 250, 400], [0, 50, 99], [0, 401, 401]], dtype=np.int32)
    T = class_thresholds(refs, 1, 0)
    assert all((T == S - 1).any() and (T == E).any() for _, S, E in refs.tolist())
    assert len(np.unique(T)) < len(T)                                    # E_j = S_k - 1: equal thresholds of two regions
    co = np.unique(np.concatenate([[E - 1, E, E + 1, S - 2, S - 1, S, S + 1] for _, S, E in refs.tolist()]))
    assert set(T.tolist()) <= set(co.tolist())
    a, b = np.meshgrid(co, co, indexing="ij")
    yield Case("D-all-pairs", refs, 1, tri(0, a[a <= b], b[a <= b]), None, READS_SORTED)
    pts = np.repeat(co, -(-2 * STEP // len(co)))
    assert len(pts) >= 2 * STEP
    yield Case("D-points-1bp", refs, 1, tri(0, pts, pts), None, READS_SORTED)
    yield Case("D-points-len100", refs, 1, tri(0, pts, pts + 100), None, READS_SORTED)
    yield Case("D-points-len1", refs, 1, tri(0, pts, pts + 1), None, READS_SORTED)
    for r in D_RUNS:
        refs = d_runs(r)
        T = class_thresholds(refs, 1, 0)
        assert (T == 1000).sum() == r and (T == 1999).sum() == r
        s = 900 + 3 * np.arange(2 * STEP)
        for kind, e in (("eq", s + 36), ("uneq", s + 36 + np.arange(len(s)) % 3), ("on", s)):
            case = Case("D-run%d-%s" % (r, kind), refs, 1, tri(0, s, e), None, READS_SORTED)
            assert case.reads[0, 2] < 1000 and case.reads[STEP - 1, 1] > 1000 and case.reads[-1, 1] > 1999   # the runs lie inside steps
            yield case
    assert {KSLOTS - 1, KSLOTS, KSLOTS + 1, 2 * KSLOTS, 3 * KSLOTS, 3 * KSLOTS + 1} <= set(D_RUNS)
    refs = d_runs(64)
    n = 2 * STEP
    for v in (999, 1000, 1001, 1999, 2000):                              # every read one coordinate: below, on and above a run
        yield Case("D-every-read-%d" % v, refs, 1, tri(0, np.full(n, v), np.full(n, v)), None, READS_SORTED)
    yield Case("D-every-read-spans-the-class", refs, 1, tri(0, np.full(n, 1), np.full(n, 5000)), None, READS_SORTED)


# ---- E: spread and coordinate limits -------------------------------------------------------------------------------------------
E_KBASE = (1, (1 << 31) - (1 << 25))


def e_refs(lo, hi, extra=()):
    ts = np.concatenate([spread(lo, hi, 90), np.asarray(extra, dtype=np.int64)])
    return regions_of(ts, far=hi + 50)


def family_e():
    i = np.arange(STEP)
    for kb in E_KBASE:
        for d in (-1, 0, 1):
            X = SPREAD_STEP + d
            # the starts of the first step spread X, its ends 255; a plain step follows
            s = np.concatenate([kb + i, kb + X + 1 + i])
            s[STEP - 1] = kb + X
            e = kb + X + 10 + np.arange(2 * STEP)
            case = Case("E-step-starts-spread%+d-kbase%d" % (d, kb), e_refs(kb, kb + X + 600, (kb + X - 1, kb + X, kb + X + 1)), 1, tri(0, s, e), None, READS_SORTED)
            assert case.reads[STEP - 1, 1] - case.reads[0, 1] == X and case.reads[STEP - 1, 2] - case.reads[0, 2] < SPREAD_STEP
            yield case
            s = kb + np.arange(2 * STEP)
            e = np.concatenate([kb + 600 + i, kb + 600 + X + 1 + i])
            e[STEP - 1] = kb + 600 + X
            case = Case("E-step-ends-spread%+d-kbase%d" % (d, kb), e_refs(kb, kb + X + 1200, (kb + 600 + X - 1, kb + 600 + X, kb + 600 + X + 1)), 1, tri(0, s, e), None, READS_SORTED)
            assert case.reads[STEP - 1, 2] - case.reads[0, 2] == X and case.reads[STEP - 1, 1] - case.reads[0, 1] < SPREAD_STEP
            yield case
            # the same with all keys but the first at the far end: the 32-bit prefix sums of the relative keys come to 255 X
            s = np.concatenate([[kb], np.full(STEP - 1, kb + X), kb + X + 1 + i])
            case = Case("E-step-starts-far%+d-kbase%d" % (d, kb), e_refs(kb, kb + X + 600, (kb + X - 1, kb + X, kb + X + 1)), 1, tri(0, s, kb + X + 10 + np.arange(2 * STEP)), None, READS_SORTED)
            assert (case.reads[1:STEP, 1].astype(np.int64) - case.reads[0, 1]).sum() == (STEP - 1) * X
            yield case
            e = np.concatenate([[kb + 600], np.full(STEP - 1, kb + 600 + X), kb + 600 + X + 1 + i])
            case = Case("E-step-ends-far%+d-kbase%d" % (d, kb), e_refs(kb, kb + X + 1200, (kb + 600 + X - 1, kb + 600 + X, kb + 600 + X + 1)), 1, tri(0, kb + np.arange(2 * STEP), e), None, READS_SORTED)
            assert (case.reads[1:STEP, 2].astype(np.int64) - case.reads[0, 2]).sum() == (STEP - 1) * X
            yield case
            X = SPREAD_CHUNK + d
            for n in (CHUNK, 2 * CHUNK):
                s = np.concatenate([[kb], np.full(CHUNK - 1, kb + X), kb + X + 1 + np.arange(n - CHUNK)])
                case = Case("E-chunk-far%+d-kbase%d-n%d" % (d, kb, n), e_refs(kb, kb + X + 600, (kb + X - 1, kb + X, kb + X + 1)), 1, tri(0, s, s + 10), None, READS_SORTED)
                assert (case.reads[1:CHUNK, 1].astype(np.int64) - case.reads[0, 1]).sum() == (CHUNK - 1) * X and case.reads[-1, 2] <= TOP
                yield case
            for n in (CHUNK, 2 * CHUNK):
                s = kb + np.arange(n)
                s[CHUNK - 1:] += X - (CHUNK - 1)
                case = Case("E-chunk-spread%+d-kbase%d-n%d" % (d, kb, n), e_refs(kb, kb + X + 600, (kb + X - 1, kb + X, kb + X + 1)), 1, tri(0, s, s + 10), None, READS_SORTED)
                assert case.reads[CHUNK - 1, 1] - case.reads[0, 1] == X and case.reads[-1, 2] <= TOP
                yield case
    assert (STEP - 1) * (SPREAD_STEP - 1) > 1 << 29 and (CHUNK - 1) * (SPREAD_CHUNK - 1) > 1 << 29      # (a limit twice as wide would pass 2^31 there)
    # reads and regions that end at the largest coordinate each may have
    s = TOP - 1000 + 3 * np.arange(2 * STEP - 200)
    j = np.arange(70)
    refs = np.concatenate([tri(0, [TOP - 500, TOP - 900, TOP - 5, REF_TOP], [REF_TOP, TOP - 100, REF_TOP, REF_TOP]), tri(0, TOP - 1000 + 10 * j, TOP - 996 + 10 * j)])
    yield Case("E-top", refs, 1, tri(0, s, np.minimum(s + 400, TOP)), None, READS_SORTED)
    yield Case("E-top-eq", refs, 1, tri(0, s[s + 36 <= TOP], s[s + 36 <= TOP] + 36), None, READS_SORTED)
    # reads of one length 2^30 / 2^31 - 4: the shifted window against kLo and kHi, over a class whose first and last windows hold sentinels
    j = np.arange(40)
    for len0 in (1 << 30, (1 << 31) - 4):
        s = 1 + (3 * np.arange(2 * STEP) if len0 == 1 << 30 else np.arange(2 * STEP) // STEP)
        hb = min(len0 - 500, TOP - 900)
        refs = np.concatenate([tri(0, 5 + 20 * j, 12 + 20 * j), tri(0, hb + 20 * j, hb + 20 * j + 7),
                               tri(0, [1, 2, 1, REF_TOP - 1, TOP - 8, 0, -7], [1, 5, REF_TOP, REF_TOP, REF_TOP - 1, REF_TOP, 3])])
        case = Case("E-len0-%d" % len0, refs, 1, tri(0, s, s + len0), None, READS_SORTED)
        T = class_thresholds(refs, 1, 0)
        assert case.reads[:, 2].max() <= TOP and (case.reads[:, 2] - case.reads[:, 1] == len0).all() and rank(T, case.reads[0, 1]) < KSLOTS and len(T) - rank(T, case.reads[-1, 2]) < KSLOTS
        yield case
    # reads with s <= 0 < e; regions with S <= 0 (S - 1 negative) and with E <= 0 (they never count)
    s = -50 + np.arange(2 * STEP) // 2
    refs = np.array([[0, -5, 10], [0, 0, 7], [0, -9, -2], [0, -3, 0], [0, 1, 3], [0, -100, 50], [0, 20, 30], [0, -60, 1], [0, 0, 1], [0, 150, 260]], dtype=np.int32)
    case = Case("E-negative-starts", refs, 1, tri(0, s, s + 60), None, READS_SORTED)
    assert (case.reads[:, 2] > 0).all() and (case.reads[:, 1] <= 0).sum() > 64 and (~taking_part(refs)).sum() == 2
    assert class_thresholds(refs, 1, 0).min() < -1
    yield case


# ---- F: what refuses a step, one cause at a time -------------------------------------------------------------------------------
F_POS = (0, 1, 63, 64, 127, 128, 191, 192, 255)
F_KINDS = ("other-class", "empty-class", "class-1", "class-n", "zero-length", "inverted2", "inverted1000", "start-descent", "end-descent", "unequal")
F_N = 4 * STEP


def f_case(kind, pos):
    i = np.arange(F_N)
    reads = tri(0, 5000 + 10 * i, 5000 + 10 * i + 36).astype(np.int64)
    at = STEP + pos
    c, s, e = reads[at]
    reads[at] = {"other-class": (1, s, e), "empty-class": (2, s, e), "class-1": (-1, s, e), "class-n": (3, s, e), "zero-length": (0, s, s - 1),
                 "inverted2": (0, s, s - 2), "inverted1000": (0, s, s - 1000), "start-descent": (0, s - 505, e), "end-descent": (0, s - 10, e - 15),
                 "unequal": (0, s, e + 3)}[kind]
    S = 5003 + 77 * np.arange(130)
    refs = np.concatenate([tri(0, S, S + 50), tri(1, 5000 + 2000 * np.arange(5), 6500 + 2000 * np.arange(5))])
    return Case("F-%s-pos%d" % (kind, pos), refs, 3, reads.astype(np.int32), None, READS_SORTED)


def family_f():
    for kind in F_KINDS:
        for pos in F_POS:
            case = f_case(kind, pos)
            q = _i64(case.reads)
            clean = np.delete(q, STEP + pos, axis=0)
            assert (clean[:, 0] == 0).all() and (np.diff(clean[:, 1]) > 0).all() and (np.diff(clean[:, 2]) > 0).all() and (clean[:, 2] - clean[:, 1] == 36).all()
            info = expected_info(case)
            assert info["n_no_class"] == (kind in ("class-1", "class-n"))
            assert info["n_degenerate"] == (kind in ("inverted2", "inverted1000")) and info["first_degenerate"] == (STEP + pos if info["n_degenerate"] else None)
            if kind == "start-descent":
                assert q[STEP + pos, 1] < q[STEP + pos - 1, 1]
            if kind == "end-descent":
                assert q[STEP + pos, 1] >= q[STEP + pos - 1, 1] and q[STEP + pos, 2] < q[STEP + pos - 1, 2]
            yield case
    assert F_N >= 2 * MIN_CPW * CHUNK


# ---- G: classes and histogram tiles --------------------------------------------------------------------------------------------
G_TOTALS = (1023, 1024, 1025, 2048, 2049, 3073)
G_LANES = tuple(range(1, 64))                                            # (1, 2, 32 and 63 are the named ones)


def g_reads(counts, classes=None, gap=10, base=4000, length=36):
    """sorted reads of one length, counts[k] of them in class classes[k]; every class starts over at `base`"""
    classes = range(len(counts)) if classes is None else classes
    return np.concatenate([tri(c, base + gap * np.arange(n), base + gap * np.arange(n) + length) for c, n in zip(classes, counts)])


def g_refs(classes, m=40, span=16000):
    return np.concatenate([tri(c, 3990 + (span // m) * np.arange(m) + c, 3990 + (span // m) * np.arange(m) + 57 + 3 * c) for c in classes])


def g_tile_case(lane):
    """one class: 1025 - lane thresholds below the first key, so the first window of the first step (its slot 0 has the rank of the first
    key) has the tile border 1024 at `lane`; the step crosses 130 thresholds, the window is flushed with keys on both sides.  What a flush
    adds to the sum of the tile above the border is read only as the offset of the tiles behind that one, and a region whose two slots
    share their tile offsets loses it in a difference: so 1100 more thresholds fill a third tile, and threshold i pairs with i + n/2"""
    n = 3 * STEP
    s = B_BASE + B_GAP * np.arange(n)
    reads = tri(0, s, s + 2)
    lo, hi = both_cross(reads, 0, STEP)
    ts = np.concatenate([B_BASE - 100 - 2 * np.arange(TILE + 1 - lane), spread(lo, hi, 130), spread(hi + 50, int(s[-1]), 40),
                         int(s[-1]) + 100 + 3 * np.arange(1100 + (TILE + 1 - lane) % 2)])
    return Case("G-tile-border-lane%d" % lane, regions_split(ts), 1, reads, None, READS_SORTED)


def g_total_case(total):
    """nt + n_classes histogram slots in all; the reads run over every threshold"""
    n_classes = 1 if total % 2 else 2
    nt = total - n_classes
    per = [nt] if n_classes == 1 else [nt // 2 - 1, nt // 2 + 1] if (nt // 2) % 2 else [nt // 2, nt // 2]
    refs = np.concatenate([regions_split(4000 + 4 * np.arange(k), cls=c) for c, k in enumerate(per)])
    return Case("G-total%d" % total, refs, n_classes, g_reads([2 * STEP] * n_classes, gap=28), None, READS_SORTED)


def family_g():
    two = g_refs((0, 1))
    for at in (STEP, STEP + 1, STEP + 128, STEP + 255):                  # a class change at a step edge and inside a step
        yield Case("G-change-at%d" % at, two, 2, g_reads([at, 3 * STEP - at]), None, READS_SORTED)
    for at in (CHUNK + 1, CHUNK + 32, CHUNK + 63):                       # ... inside a chunk, no step
        yield Case("G-change-at%d" % at, two, 2, g_reads([at, 3 * CHUNK - at]), None, READS_SORTED)
    for k in (3, 5):                                                     # the third turn of a chunk: lanes on their own, a segment per lane
        for n in (CHUNK, 2 * CHUNK, 2 * STEP):
            counts = [13] * (k - 1) + [n - 13 * (k - 1)]
            case = Case("G-%d-classes-in-a-chunk-n%d" % (k, n), g_refs(range(k)), k, g_reads(counts), None, READS_SORTED)
            assert len(set(case.reads[:CHUNK, 0].tolist())) == k
            yield case
    hole = g_refs((0, 2))
    for counts in ([STEP, STEP, STEP], [STEP + 20, STEP + 7, STEP], [20, 20, 24], [300, 700, 300]):
        yield Case("G-class-without-regions-%s" % "-".join(map(str, counts)), hole, 3, g_reads(counts), None, READS_SORTED)
    three = g_refs((0, 1, 2))
    yield Case("G-classes-descending", three, 3, g_reads([300, 300, 300], classes=(2, 1, 0)), None, READS_SORTED)
    yield Case("G-classes-descending-steps", three, 3, g_reads([STEP, 2 * STEP, STEP], classes=(2, 1, 0)), None, READS_SORTED)
    for lane in G_LANES:
        case = g_tile_case(lane)
        T = class_thresholds(case.refs, 1, 0)
        for k in (1, 2):                                                 # both windows: the border's lane, and keys on either side of it
            r = rank(T, case.reads[:STEP, k])
            b0 = head_of_span(place_table(case.refs, 1), case.reads, 0)[k - 1][0]
            assert TILE - (b0 - 1) == lane and ((r >= b0) & (r < TILE)).any() == (lane > 1) and ((r >= TILE) & (r <= b0 + KSLOTS - 1)).any(), case.name
            assert r[-1] > b0 + KSLOTS                                   # the step leaves the window: it is flushed
        slot_s, slot_e = rank(T, case.refs[:, 1].astype(np.int64) - 1) >> TILE_SHIFT, rank(T, case.refs[:, 2]) >> TILE_SHIFT
        assert ((slot_s <= 1) & (slot_e == 2)).any() and len(T) > 2 * TILE   # regions that read the offset of the tile behind the border's
        yield case
    assert {1, 2, 32, 63} <= set(G_LANES)
    for total in G_TOTALS:
        case = g_total_case(total)
        T, seg = thresholds(case.refs, case.n_classes)
        assert len(T) + case.n_classes == total and all(rank(T[seg[c]:seg[c + 1]], case.reads[case.reads[:, 0] == c][-1, 1]) == seg[c + 1] - seg[c] for c in range(case.n_classes))
        yield case
    # a class whose base slot (seg[c] + c - 1) lies in the tile below the one of its regions' slots (seg[c] + c + rank)
    refs = np.concatenate([regions_of(4000 + 4 * np.arange(510), cls=0), regions_of(4000 + 4 * np.arange(512), cls=1), regions_of(4000 + 40 * np.arange(40), cls=2)])
    T, seg = thresholds(refs, 3)
    assert seg[2] + 2 - 1 == TILE - 1 and seg[2] + 2 == TILE
    yield Case("G-class-base-in-the-tile-below", refs, 3, g_reads([2 * STEP, 2 * STEP, STEP]), None, READS_SORTED)


# ---- I: the partition kernel ---------------------------------------------------------------------------------------------------
# (a region that takes part adds two thresholds, so a class has an even number of them: the odd sizes next to the cuts are out of reach
#  and their even neighbours stand in)
I_NT = (2, 2046, 2048, 2050, 2558, 2560, 2562, 4094, 4096, 4098, 4606, 4608, 4610)
I_ODD_NT_OUT_OF_REACH = (1, 2047, 2049, 2559, 2561, 4095, 4097, 4607, 4609)


def i_case(nt, kind="plain"):
    rng = np.random.default_rng(nt)
    T = 100 + 4 * np.arange(nt)
    if kind == "equal-over-the-cut" and nt > BKT_E + 8:
        T[BKT_E - 8:BKT_E + 8] = T[BKT_E - 8]
    if kind == "bucket-of-equal" and nt >= 2 * BKT_E:
        T[BKT_E:2 * BKT_E] = T[BKT_E]
    refs = np.concatenate([regions_split(T, 0), tri(1, 50 + 30 * np.arange(60), 70 + 30 * np.arange(60))])
    top = int(T[-1]) + 40
    rows = []
    for lo in range(0, nt, BKT_E):                                       # the bucket [lo, hi) and its slice [lo, sl)
        hi, sl = min(lo + BKT_E, nt), min(lo + BKT_T, nt)
        starts = [T[hi - 1], T[hi - 1] - 1, T[lo], T[lo] - 1, T[lo] + 1]  # the bucket's last slot; at, below and above its lowest threshold
        ranks = [sl - lo - 1, sl - lo, sl - lo + 1, sl - lo + 2, nt - lo, nt - lo - 1]   # the end's rank inside the slice: nS - 1, nS, nS + 1, far beyond
        ends = [int(T[lo + r]) if lo + r < nt else int(T[-1]) + 1 for r in ranks if 0 <= lo + r <= nt] + [top]
        rows += [(0, int(s), int(e)) for s in starts for e in ends if s <= e]
    s = rng.integers(60, top, size=1200)
    body = tri(0, s, s + rng.choice([0, 3, 50, 4000, 12000], size=len(s)))
    s1 = rng.integers(1, 2000, size=150)
    odd = np.array([[0, 500, 499], [0, 600, 590], [1, 100, 99], [1, 300, 200], [0, int(T[hi - 1]), int(T[hi - 1]) - 1], [0, int(T[0]), int(T[0]) - 7]], dtype=np.int32)
    reads = np.concatenate([np.array(rows, dtype=np.int32).reshape(-1, 3), body, tri(1, s1, s1 + 25), odd])
    return Case("I-nt%d-%s" % (nt, kind), refs, 2, reads[rng.permutation(len(reads))], None, READS_UNSORTED)


def family_i():
    beyond = {True: 0, False: 0}                                         # reads that end at or beyond a slice, by "the slice ends with the class"
    for nt in I_NT:
        case = i_case(nt)
        T, seg = thresholds(case.refs, 2)
        assert seg[1] == nt and seg[2] - seg[1] == 120
        q = _i64(case.reads)
        q = q[(q[:, 0] == 0) & (q[:, 1] <= q[:, 2])]
        rs, re_ = rank(T[:nt], q[:, 1]), rank(T[:nt], q[:, 2])
        for lo in range(0, nt, BKT_E):
            hi, sl = min(lo + BKT_E, nt), min(lo + BKT_T, nt)
            last = rs == hi - 1                                          # reads that start in the bucket's last slot below the cut
            want = {sl - 1, sl} | ({sl + 1} if sl + 1 <= nt else set()) | {nt}
            assert want <= set(re_[last].tolist()), (case.name, lo)
            assert (rs == lo).any()
            mine = (rs >= lo) & (rs < hi) if hi < nt else rs >= lo       # the bucket's reads: by their start, the last bucket takes the rest
            assert (re_[mine] >= sl).any(), (case.name, lo)
            beyond[sl == nt] += int((re_[mine] >= sl).sum())
        assert oracle_takes(case).mean() > 0.9
        yield case
    assert beyond[True] and beyond[False]                                # the global search above the slice, and the slice that needs none
    assert {BKT_E, BKT_E + 2, BKT_T, BKT_T + 2, 2 * BKT_E, 2 * BKT_E + 2, BKT_E + BKT_T, BKT_E + BKT_T + 2} <= set(I_NT)
    for nt in (2562, 4098):
        case = i_case(nt, "equal-over-the-cut")
        T = class_thresholds(case.refs, 2, 0)
        assert T[BKT_E - 1] == T[BKT_E] and (T == T[BKT_E]).sum() == 16
        yield case
    for nt in (4096, 4610):
        case = i_case(nt, "bucket-of-equal")
        T = class_thresholds(case.refs, 2, 0)
        assert T[BKT_E] == T[2 * BKT_E - 1] and T[BKT_E - 1] < T[BKT_E]
        yield case


GENERATORS = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f, "G": family_g, "I": family_i}


@functools.lru_cache(maxsize=None)
def family(fam):
    """the cases of one family without weights (generated once per process; running a generator to its end checks the family's aim)"""
    out = list(GENERATORS[fam]())
    assert len({c.name for c in out}) == len(out)
    for c in out:
        assert len(c.reads) <= 4200 and len(c.refs) <= 5200, c.name
        for a in (c.refs, c.reads):
            a.setflags(write=False)
    return out


def with_weights(case, variant):
    return case._replace(name="%s/%s" % (case.name, variant), weights=weights_for(case.name, len(case.reads), variant))


def cases(fam, variant="none"):
    return [with_weights(c, variant) for c in family(fam)]


@functools.lru_cache(maxsize=None)
def wanted(fam):
    """brute() of every case of a family in every weight variant, computed once: {case name: {variant: coverage}}"""
    out = {}
    for c in family(fam):
        ws = [weights_for(c.name, len(c.reads), v) for v in VARIANTS]
        res = brute_multi(c.refs, c.reads, ws)
        for r in res:
            r.setflags(write=False)
        out[c.name] = dict(zip(VARIANTS, res))
    return out
