"""Cases for the window scans (scan_hist_kernel + scan_window_kernel in csrc/gtx_kernels.hip, the owner-computes pass in csrc/gtx_scanown.hip,
bucket_scanhist_kernel + scan_zero_edges_kernel in csrc/gtx_bucket.hip) that sit on their seams instead of in the interior of their paths:
the 256-read step and the uniform-class fast path, the reciprocal division at the ends of a micro-window and of the coordinate range, the
window tile and the sliding run of one thread, the 1024-slot LDS tile of the histogram pass and its run pre-aggregation, the search keys
and the order check of the owner blocks, and the cuts between parts and buckets of the partition path.

Shared by tests/test_scan_cases_cpu.py (no GPU: the references against each other and against the oracle's two scanners, every family's
aim, the pinned constants) and tests/test_gpu_scan_seams.py (+ its child tests/scan_seams_child.py).  brute() is the definition of the
reduction, brute_py() the same in Python integers.  SRC pins the kernel constants the cases aim at: name -> (source file under csrc/,
regular expression, the values of its groups).  The route rules (who takes the partition path, the bucket width, fused or not) are pinned
in tests/switch_points.py and asked through `gtx_packtool route`; they are not restated here."""
import collections
import functools
import zlib

import numpy as np

READS_SORTED, READS_UNSORTED, ZERO_LENGTH_OK = 1, 16, 4

STEP = 256                      # reads per step of scan_hist_kernel (R = 4 registers of 64)
SCAN_TILE = 1024                # micro-window counters of a wave's LDS tile
WIN_PER = 8                     # windows one thread of scan_window_kernel slides over
WIN_TILE = 256 * WIN_PER        # windows per block of scan_window_kernel
WIN_MAX_COMB = 2048             # above: direct sums
OWN_THREADS, OWN_U = 256, 4     # the owner loop takes OWN_U * OWN_THREADS reads a turn
OWN_TURN = OWN_THREADS * OWN_U
OWN_MAX_TILE = 8192
OWN_FLOOR, OWN_DEFAULT = 64, 2048
BINS32, BINS64 = 30720, 15360   # micro-windows per part of the partition path, unweighted / weighted
BKT_MIN_PER = 16384             # micro-windows per bucket at the least (tests/switch_points.py pins it)
FUSED_MAX_COMB = 64
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
MAX_LEN = INT32_MAX             # class lengths are int32: the largest the library accepts
TOP = INT32_MAX                 # the largest coordinate of a read

SRC = {
    "SCAN_TILE": ("gtx_kernels.hip", r"static constexpr int kScanTile = (\d+);", (SCAN_TILE,)),
    "WIN_PER": ("gtx_kernels.hip", r"static constexpr int kWinPer = (\d+);", (WIN_PER,)),
    "WIN_TILE": ("gtx_kernels.hip", r"static constexpr int kWinTile = (\d+) \* kWinPer;", (WIN_TILE // WIN_PER,)),
    "WIN_MAX_COMB": ("gtx_kernels.hip", r"static constexpr int kWinMaxComb = (\d+);", (WIN_MAX_COMB,)),
    "WIN_DIRECT_RULE": ("gtx_kernels.hip", r"if \(a\.comb > kWinMaxComb\) \{", ()),
    "STEP_R": ("gtx_kernels.hip", r"scan_hist_kernel\(const Tri \*__restrict__ reads, const int \*__restrict__ weights, i64 n, ScanArgs a, const int \*__restrict__ runIf\)\n"
               r"\{\n[^\n]*\n  constexpr int R = (\d+);", (STEP // 64,)),
    "OWN_THREADS": ("gtx_scanown.hip", r"static constexpr int kOwnThreads = (\d+);", (OWN_THREADS,)),
    "OWN_MAX_TILE": ("gtx_scanown.hip", r"static constexpr int kOwnMaxTile = (\d+);", (OWN_MAX_TILE,)),
    "OWN_U": ("gtx_scanown.hip", r"constexpr int U = (\d+);", (OWN_U,)),
    "OWN_REFUSAL": ("gtx_scanown.hip", r"if \(comb > kOwnMaxTile / (\d+) \|\| totalMicro <= 0\) return 0;", (OWN_MAX_TILE // WIN_MAX_COMB,)),
    "OWN_DEFAULT": ("gtx_scanown.hip", r"getenv\(\"GTX_SCAN_OWN_TILE\"\) \? atoll\(getenv\(\"GTX_SCAN_OWN_TILE\"\)\) : (\d+);", (OWN_DEFAULT,)),
    "OWN_FLOOR": ("gtx_scanown.hip", r"if \(t < 2 \* comb\) t = 2 \* comb;\n  if \(t < (\d+)\) t = (\d+);\n  if \(t > kOwnMaxTile\) t = kOwnMaxTile;\n  int p = (\d+); while \(p < t\) p \*= 2;",
                  (OWN_FLOOR, OWN_FLOOR, OWN_FLOOR)),
    "OWN_END_RULE": ("gtx_scanown.hip", r"if \(k == nb - 1 \|\| endPos > \(i64\)INT_MAX\) end = lower_bound_reads\(reads, n, c \+ 1, INT_MIN\);", ()),
    "PART_BINS": ("gtx_bucket.hip", r"static constexpr int kScanBins32 = (\d+), kScanBins64 = (\d+);", (BINS32, BINS64)),
    "FUSED_MAX_COMB": ("gtx_bucket.hip", r"int scan_fused_max_comb\(\) \{ return (\d+); \}", (FUSED_MAX_COMB,)),
}

Case = collections.namedtuple("Case", "name reads class_len step size prep aim")
VARIANTS = ("none", "small", "signed", "zero")
FAMILIES = "ABCDEFG"
CHILD = "H"                      # family G's cases for the child process with GTX_SCAN_BUCKETS=1


# ---- references ----------------------------------------------------------------------------------------------------------------
def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1, 3)


def layout(class_len, step, size):
    """(nMicro, nWin, offsets, total) per class"""
    ln = np.maximum(np.asarray(class_len, dtype=np.int64), 0)
    nm, comb = ln // step, size // step
    nw = np.where(nm < comb, 0, nm - comb + 1)
    off = np.concatenate([[0], np.cumsum(nw)])
    return nm, nw, off[:-1], int(off[-1])


def positions(reads, prep, sorted_rule):
    """(counts, pos) per read: whether it counts, and the position that places it"""
    q = _i64(reads)
    s, e = q[:, 1], q[:, 2]
    ok = np.ones(len(q), dtype=bool) if sorted_rule else (s <= e) & (e > 0)
    d = e - s
    pos = s + np.sign(d) * (np.abs(d) // 2) if prep == "c" else s.copy()           # C's truncating division
    if sorted_rule:
        pos = np.maximum(pos, 1)
    return ok & (pos >= 1), pos


def brute_multi(reads, class_len, step, size, prep, ws, sorted_rule=False):
    """brute() for several weight vectors over one geometry"""
    q = _i64(reads)
    nm, nw, off, tot = layout(class_len, step, size)
    comb = size // step
    ok, pos = positions(q, prep, sorted_rule)
    outs = []
    for w in ws:
        wt = (np.ones(len(q), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)).astype(np.uint64)
        out = np.zeros(tot, dtype=np.uint64)
        for c in range(len(nm)):
            if nw[c] == 0:
                continue
            m = (pos - 1) // step
            take = ok & (q[:, 0] == c) & (m < nm[c])
            micro = np.zeros(int(nm[c]), dtype=np.uint64)
            np.add.at(micro, m[take], wt[take])                                      # uint64: exactly mod 2^64
            cs = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(micro, dtype=np.uint64)])
            out[off[c]:off[c] + nw[c]] = cs[comb:comb + nw[c]] - cs[:nw[c]]          # sum(micro[k : k + comb]) mod 2^64
        outs.append(out)
    return outs


def brute(reads, class_len, step, size, prep="1", weights=None, sorted_rule=False):
    """out[k] = sum of the weights of the reads whose position falls into the micro-windows k .. k + comb - 1 of its class, mod 2^64"""
    return brute_multi(reads, class_len, step, size, prep, [weights], sorted_rule)[0]


def brute_py_multi(reads, class_len, step, size, prep, ws, sorted_rule=False):
    """the same in Python integers, reduced mod 2^64 at the end"""
    q = _i64(reads).tolist()
    comb = size // step
    placed = []                                                                      # (read index, class, micro-window)
    for i, (c, s, e) in enumerate(q):
        if not sorted_rule and not (s <= e and e > 0):
            continue
        pos = s
        if prep == "c":
            d = e - s
            pos = s + (d // 2 if d >= 0 else -((-d) // 2))
        if pos < 1:
            if not sorted_rule:
                continue
            pos = 1
        placed.append((i, c, (pos - 1) // step))
    outs = []
    for w in ws:
        out = []
        for c, ln in enumerate(int(x) for x in class_len):
            n_micro = max(ln, 0) // step
            n_win = n_micro - comb + 1 if n_micro >= comb else 0
            if n_win == 0:
                continue
            micro = [0] * n_micro
            for i, rc, m in placed:
                if rc == c and m < n_micro:
                    micro[m] += 1 if w is None else int(w[i])
            run = sum(micro[:comb])
            out.append(run)
            for k in range(1, n_win):
                run += micro[k + comb - 1] - micro[k - 1]
                out.append(run)
        outs.append(np.array([x % (1 << 64) for x in out], dtype=np.uint64))
    return outs


def brute_py(reads, class_len, step, size, prep="1", weights=None, sorted_rule=False):
    return brute_py_multi(reads, class_len, step, size, prep, [weights], sorted_rule)[0]


def in_order(reads):
    """(class, start) order, as the owner pass checks it and the oracle's sorted scanner needs it"""
    q = _i64(reads)
    key = q[:, 0] * (1 << 33) + (q[:, 1] + (1 << 31))
    return bool((np.diff(key) >= 0).all())


def oracle_takes(case):
    """the reads the oracle knows a class for"""
    q = _i64(case.reads)
    return (q[:, 0] >= 0) & (q[:, 0] < len(case.class_len))


def weights_for(name, n, variant):
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (name, variant)).encode()))
    if variant == "none":
        return None
    if variant == "small":
        return rng.integers(0, 10, size=n).astype(np.int32)
    if variant == "zero" or n == 0:
        return np.zeros(n, dtype=np.int32)
    w = rng.integers(INT32_MIN, INT32_MAX + 1, size=n).astype(np.int32)
    ext = rng.integers(0, n, size=max(2, n // 16))
    w[ext[::2]] = INT32_MIN
    w[ext[1::2]] = INT32_MAX
    w[0] = INT32_MIN
    w[-1] = INT32_MAX if n > 1 else INT32_MIN
    return w


def own_tile(cap, comb):
    """windows per owner block for GTX_SCAN_OWN_TILE=cap (None: unset) with GTX_SCAN_OWN_ALWAYS=1; 0 = the pass declines (scan_own_tile)"""
    if comb > OWN_MAX_TILE // 4:
        return 0
    t = min(max(OWN_DEFAULT if cap is None else cap, 2 * comb, OWN_FLOOR), OWN_MAX_TILE)
    p = OWN_FLOOR
    while p < t:
        p *= 2
    return min(p, OWN_MAX_TILE)


def own_bounds(reads, class_len, step, size, tile):
    """what scan_bounds_kernel finds on reads in order: per block (class, k, own0, cnt1, end key beyond INT_MAX), and the end of the stream"""
    q = _i64(reads)
    assert in_order(q)
    key = q[:, 0] * (1 << 33) + (q[:, 1] + (1 << 31))
    nm, nw, _, _ = layout(class_len, step, size)
    comb = size // step

    def lb(c, p):
        return int(np.searchsorted(key, c * (1 << 33) + (p + (1 << 31)), side="left"))
    out = []
    for c in range(len(nm)):
        nb = -(-int(nw[c]) // tile)
        for k in range(nb):
            own0 = 0 if not out else lb(c, INT32_MIN if k == 0 else k * tile * step + 1)
            end_pos = ((k + 1) * tile + comb - 1) * step + 1
            cnt1 = lb(c + 1, INT32_MIN) if k == nb - 1 or end_pos > INT32_MAX else lb(c, end_pos)
            out.append((c, k, own0, cnt1, end_pos > INT32_MAX))
    return out, len(q)


# ---- builders ------------------------------------------------------------------------------------------------------------------
def tri(c, s, e):
    s = np.atleast_1d(np.asarray(s, dtype=np.int64))
    out = np.empty((len(s), 3), dtype=np.int64)
    out[:, 0], out[:, 1], out[:, 2] = c, s, e
    assert len(s) == 0 or (out[:, 1:].min() >= INT32_MIN and out[:, 1:].max() <= INT32_MAX)
    return out.astype(np.int32)


def cnt(m):
    """reads per micro-window m: neighbours differ, and no window of the sizes used here sums to a constant (the period is 15)"""
    return 1 + m % 3 + 3 * (m % 5 == 0)


def fill(cls, ms, step, ext=35, mult=1):
    """mult * cnt(m) reads of class cls in every micro-window m of ms, spread from its first position m * step + 1 to its last"""
    rows = []
    for m in sorted(set(int(x) for x in ms)):
        k = mult * cnt(m)
        for i in range(k):
            rows.append(m * step + 1 + (i * (step - 1)) // max(k - 1, 1))
    s = np.array(rows, dtype=np.int64)
    return tri(cls, s, np.minimum(s + ext, INT32_MAX)) if len(rows) else np.zeros((0, 3), dtype=np.int32)


def at_positions(cls, ps, ext=35):
    """cnt(j) reads at the j-th position of ps"""
    s = np.array([p for j, p in enumerate(ps) for _ in range(cnt(j)) if INT32_MIN <= p <= INT32_MAX], dtype=np.int64)
    return tri(cls, s, np.minimum(s + ext, INT32_MAX))


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.int32).reshape(-1, 3) for p in parts])


def ordered(reads):
    q = _i64(reads)
    return np.ascontiguousarray(reads[np.lexsort((q[:, 1], q[:, 0]))])


def near(points, r, lo, hi):
    """every micro-window within r of a point, inside [lo, hi)"""
    return sorted({m for p in points for m in range(p - r, p + r + 1) if lo <= m < hi})


def centred(case):
    """the twin for preprocess 'c': every read that counts is replaced by one of another length whose centre is the old start"""
    q = _i64(case.reads).copy()
    valid = (q[:, 1] <= q[:, 2]) & (q[:, 2] > 0) & (q[:, 1] >= 1)
    h = 1 + np.arange(len(q)) % 7
    odd = np.arange(len(q)) % 2
    h = np.where(q[:, 1] + h + odd > INT32_MAX, 0, h)
    odd = np.where(h == 0, 0, odd)
    s = q[:, 1].copy()
    q[valid, 1] = (s - h)[valid]
    q[valid, 2] = (s + h + odd)[valid]
    q[~valid & (q[:, 1] < 1) & (q[:, 2] > 0), 2] = 1                                      # a start below 1 that counts: its centre stays below 1
    twin = case._replace(name=case.name + "-centre", reads=q.astype(np.int32), prep="c")
    ok, pos = positions(twin.reads, "c", False)
    ok0, pos0 = positions(case.reads, "1", False)
    assert (ok == ok0).all() and (pos[ok] == pos0[ok]).all()
    return twin


def micro_of(case, sorted_rule=False):
    """(class, micro-window) of the reads that count (-1, -1 for the others)"""
    q = _i64(case.reads)
    nm = layout(case.class_len, case.step, case.size)[0]
    ok, pos = positions(q, case.prep, sorted_rule)
    known = (q[:, 0] >= 0) & (q[:, 0] < len(nm))
    m = (pos - 1) // case.step
    ok = ok & known
    ok[ok] &= m[ok] < nm[q[ok, 0]]
    return np.where(ok, q[:, 0], -1), np.where(ok, m, -1)


def has_read_at(case, cls, p):
    q = _i64(case.reads)
    return bool(((q[:, 0] == cls) & (q[:, 1] == p)).any())


# ---- A: reads per step, classes in a step ----------------------------------------------------------------------------------------
A_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
A_CHANGE_LANES = (0, 63, 64, 255, 256)
A_ODD_KINDS = ("other-class", "class-neg", "class-n", "class-max", "inverted", "non-positive", "zero-length")
A_ODD_LANES = (0, 100, 255)
A_LEN, A_STEP, A_SIZE = (25 * 600 + 7, 25 * 300, 25 * 500 + 24), 25, 50


def family_a():
    stream = fill(0, range(600), A_STEP)
    assert len(stream) > max(A_SIZES)
    for n in A_SIZES:
        yield Case("A-n%d" % n, stream[:n].copy(), A_LEN, A_STEP, A_SIZE, "1", "n = %d reads" % n)
    for lane in A_CHANGE_LANES:
        r = cat(fill(0, range(600), A_STEP)[:STEP + lane], fill(1, range(300), A_STEP)[:2 * STEP - lane])
        assert len(r) == 3 * STEP and r[STEP + lane - 1, 0] == 0 and r[STEP + lane, 0] == 1 and in_order(r)
        yield Case("A-change-lane%d" % lane, r, A_LEN, A_STEP, A_SIZE, "1", "the class changes at lane %d of the second step" % lane)
    for kind in A_ODD_KINDS:
        for lane in A_ODD_LANES:
            r = stream[:2 * STEP].copy()
            i = STEP + lane
            s = int(r[i, 1])
            r[i] = {"other-class": (1, s, s + 35), "class-neg": (-1, s, s + 35), "class-n": (len(A_LEN), s, s + 35), "class-max": (INT32_MAX, s, s + 35),
                    "inverted": (0, s, s - 1), "non-positive": (0, -40, 0), "zero-length": (0, s, s)}[kind]
            others = np.delete(r[STEP:], lane, axis=0)
            assert (others[:, 0] == 0).all() and (others[:, 1] <= others[:, 2]).all()          # an otherwise uniform, valid step
            yield Case("A-odd-%s-lane%d" % (kind, lane), r, A_LEN, A_STEP, A_SIZE, "1", "one %s read at lane %d of a uniform step" % (kind, lane))
    # the centre with C's truncating division: inverted reads of odd and even length count under the sorted scanner's rule
    r = stream[:STEP + 7].copy()
    r[3], r[70], r[STEP + 2] = (0, 504, 497), (0, 505, 497), (0, 38, 13)      # centres 501, 501 and 26: one position lower if the division floored
    yield Case("A-centre-truncates", r, A_LEN, A_STEP, A_SIZE, "c", "inverted reads under preprocess c (the division truncates towards zero)")


# ---- B: the division -------------------------------------------------------------------------------------------------------------
B_STEPS = (1, 2, 3, 7, 25, 1000, 4097, 65536, 65537, (1 << 20) + 1, (1 << 30) + 1)
B_LIMIT_FROM = 65536              # from this step on the class has the largest length there is (a few thousand micro-windows)


def b_case(step):
    ln = MAX_LEN if step >= B_LIMIT_FROM else 40 * step + step - 1
    n_micro = ln // step
    size = 2 * step if 2 * step <= INT32_MAX and n_micro >= 2 else step
    ps = [q * step + d for q in (0, 1, 2, n_micro - 1, n_micro) for d in (0, 1, 2)] + [ln, ln + 1, TOP, TOP - 1]
    ps = sorted(set(p for p in ps if p <= TOP))
    lens = (ln, 3 * step + 1 if 3 * step + 1 <= INT32_MAX else step)
    r = cat(at_positions(0, ps), at_positions(1, [1, step, step + 1, 3 * step, 3 * step + 1]))
    return Case("B-step%d" % step, ordered(r), lens, step, size, "1", "reads at q * %d + {0, 1, 2} and at the top of the range" % step), ps


def family_b():
    for step in B_STEPS:
        case, ps = b_case(step)
        n_micro = case.class_len[0] // step
        for q in (0, 1, 2, n_micro - 1, n_micro):
            for d in (0, 1, 2):
                assert q * step + d > TOP or has_read_at(case, 0, q * step + d), (step, q, d)
        assert has_read_at(case, 0, TOP) and (case.class_len[0] + 1 > TOP or has_read_at(case, 0, case.class_len[0] + 1))
        assert in_order(case.reads) and n_micro <= 1 << 15
        if step >= B_LIMIT_FROM:
            assert case.class_len[0] == MAX_LEN
        yield case
        yield centred(case)


def reciprocal_worst(step, xs):
    """x // step - ((x * floor(2^32 / step)) >> 32) over xs: (smallest, largest) -- scan_slot's two fix-ups assume 0 .. 1"""
    inv = (1 << 32) // step
    d = [x // step - ((x * inv) >> 32) for x in xs]
    return min(d), max(d)


# ---- C: window sums --------------------------------------------------------------------------------------------------------------
C_COMB = (1, 2, 8, 9, 63, 64, 65, 2047, 2048, 2049)
C_NWIN = (0, 1, 2, 2047, 2048, 2049, 4097)
C_STEP = 2


def c_case(comb, n_win):
    n_micro = comb - 1 + n_win
    seams = [0, comb - 1, comb, n_win - 1, n_win, n_micro - 1, WIN_TILE - 1, WIN_TILE, WIN_TILE + comb - 1, 2 * WIN_TILE, 2 * WIN_TILE + comb - 1]
    ms = set(near(seams, 10, 0, n_micro)) | set(range(0, n_micro, 7)) | (set(range(n_micro)) if n_micro <= 300 else set())
    side = 40 + comb                                                                 # a class beside it, so that the offsets count
    lens = (n_micro * C_STEP + 1, side * C_STEP)
    r = cat(fill(0, ms, C_STEP), fill(1, range(0, side, 3), C_STEP))
    if (comb + n_win) % 2:                                                           # the aimed class second
        lens, r = lens[::-1], cat(r[r[:, 0] == 1], r[r[:, 0] == 0])
        r[:, 0] ^= 1
    return Case("C-comb%d-nwin%d" % (comb, n_win), r, lens, C_STEP, comb * C_STEP, "1", "comb %d, a class of %d windows" % (comb, n_win))


def family_c():
    for comb in C_COMB:
        for n_win in C_NWIN:
            case = c_case(comb, n_win)
            nm, nw, _, _ = layout(case.class_len, case.step, case.size)
            aimed = 1 if (comb + n_win) % 2 else 0
            assert nw[aimed] == n_win and nw[1 - aimed] == 41 and in_order(case.reads)
            if n_win == 0:
                assert nm[aimed] == comb - 1
            yield case


# ---- D: the LDS tile of the histogram pass -----------------------------------------------------------------------------------------
D_LEN = (6000, 6000)
D_RUNS = (1, 2, 63, 64, 65, 128)
D_RUN_LANES = (0, 1, 63)
D_SIZES = (STEP, STEP - 56)       # one whole step (the fast path) and the same reads through the tail code


def d_reads(cls_micro):
    c = np.array([x[0] for x in cls_micro], dtype=np.int64)
    m = np.array([x[1] for x in cls_micro], dtype=np.int64)
    return tri(c, m + 1, m + 36)                                                     # step 1: micro-window = position - 1


def family_d():
    def case(name, cm, aim):
        return [Case("D-%s-n%d" % (name, n), d_reads(cm[:n]), D_LEN, 1, 3, "1", aim) for n in D_SIZES]
    for base in (0, 5):
        # register 0 puts the tile at `base`; register 1 walks over base + 1023 / base + 1024; register 2 begins beyond
        cm = [(0, base)] * 10 + [(0, base + 900 + i) for i in range(54)] + [(0, base + 1020 + i // 8) for i in range(64)] + [(0, base + 1028 + i) for i in range(128)]
        m1 = [m for _, m in cm[64:128]]
        assert cm[0][1] == base and base + SCAN_TILE - 1 in m1 and base + SCAN_TILE in m1 and m1[0] < base + SCAN_TILE and cm[128][1] >= base + SCAN_TILE
        for c in case("walk-base%d" % base, cm, "micro-windows walk over base + 1023 and base + 1024 inside one register"):
            assert in_order(c.reads)
            yield c
    cm = [(0, 500 + i // 2) for i in range(70)] + [(1, 100 + i // 3) for i in range(186)]
    assert cm[69][0] == 0 and cm[70] == (1, 100) and 64 < 70 < 128
    for c in case("back-class", cm, "a class change inside a register takes the micro-windows back below the tile's base"):
        assert in_order(c.reads)
        yield c
    cm = [(0, 500 + i // 2) for i in range(70)] + [(0, 100 + i // 3) for i in range(186)]
    yield from case("back-start", cm, "reads in no order: micro-windows below the tile's base inside a register")
    cm = [(i % 2, 300 + i // 4) for i in range(STEP)]
    yield from case("alternate", cm, "two classes alternate inside every register")
    cm = [(0, 1100 * (i % 5) + i // 5) for i in range(STEP)]
    assert all(abs(cm[i + 1][1] - cm[i][1]) > SCAN_TILE for i in range(0, 60) if (i + 1) % 5)
    yield from case("apart", cm, "neighbouring reads more than a tile apart: atomics straight to the micro-window array")
    for run in D_RUNS:
        for lane in D_RUN_LANES:
            cm = [(0, 2 * i) for i in range(lane)] + [(0, 200)] * run
            cm += [(0, 300 + 2 * i) for i in range(STEP - len(cm))]
            assert cm[lane][1] == 200 and cm[lane + run - 1][1] == 200 and cm[lane + run][1] != 200 and (lane == 0 or cm[lane - 1][1] != 200)
            for c in case("run%d-lane%d" % (run, lane), cm, "a run of %d equal micro-windows from lane %d" % (run, lane)):
                assert in_order(c.reads)
                yield c


# ---- E: owner blocks -------------------------------------------------------------------------------------------------------------
E_CAPS = (64, None)               # GTX_SCAN_OWN_TILE: the floor, and unset (2048)
E_COMBS = (1, 5, 64)
E_STEP = 3
E_TOP_STEP = 1 << 20


def e_keys(case, tile):
    """the owner blocks' search keys of every class that has blocks: positions k * T * D + {0, 1} and ((k + 1) T + comb - 1) D + {0, 1}"""
    nm, nw, _, _ = layout(case.class_len, case.step, case.size)
    comb, out = case.size // case.step, []
    for c in range(len(nm)):
        for k in range(-(-int(nw[c]) // tile)):
            for p in (k * tile * case.step, ((k + 1) * tile + comb - 1) * case.step):
                out += [(c, p), (c, p + 1)]
    return out


def e_blocks_case(cap, comb):
    t = own_tile(cap, comb)
    n_wins = (t - 1, t, 0, t + 1, 2 * t, 2 * t + 1)
    n_micro = [comb - 1 + w for w in n_wins]
    lens = tuple(m * E_STEP + (c % E_STEP) for c, m in enumerate(n_micro))
    name = "E-blocks-T%d-comb%d" % (t, comb)
    proto = Case(name, None, lens, E_STEP, comb * E_STEP, "1", "blocks of %d windows: classes of T - 1, T, none, T + 1, 2T, 2T + 1 windows, reads on the search keys" % t)
    parts = []
    for c, m in enumerate(n_micro):
        pts = [0, m - 1] + [k * t + d for k in range(4) for d in (-1, 0, comb - 2, comb - 1, comb)]
        ms = set(near(pts, 2, 0, m)) | set(range(0, m, 13 if t > 64 else 5))
        parts.append(fill(c, ms, E_STEP))
        if c == 2:                                                                   # the class without windows has reads of its own, beyond its end too
            parts.append(at_positions(c, [1, 2, lens[c], lens[c] + 1, lens[c] + 50]))
    keys = e_keys(proto, t)
    for c in range(len(lens)):
        parts.append(at_positions(c, [p for kc, p in keys if kc == c and p >= 1]))
    case = proto._replace(reads=ordered(cat(*parts)))
    for c, p in keys:
        assert p < 1 or has_read_at(case, c, p), (name, c, p)
    nw = layout(lens, E_STEP, comb * E_STEP)[1]
    assert tuple(int(x) for x in nw) == n_wins
    return case, t


def e_single(name, cap, comb, lens, reads, step, aim):
    return Case("E-%s-T%d" % (name, own_tile(cap, comb)), ordered(reads), lens, step, comb * step, "1", aim)


def family_e():
    seen = set()
    for cap in E_CAPS:
        for comb in E_COMBS:
            case, t = e_blocks_case(cap, comb)
            if case.name not in seen:
                seen.add(case.name)
                yield case
        t = own_tile(cap, 2)
        lens = (3 * t + 1, 50)
        # a block with no read: nothing in the micro-windows block 1 sums
        r = cat(fill(0, range(0, t - 1), 1), fill(0, range(2 * t + 2, 3 * t), 1), fill(1, range(0, 50, 2), 1))
        c = e_single("empty-block", cap, 2, lens, r, 1, "block 1 of class 0 counts no read")
        b, _ = own_bounds(c.reads, c.class_len, 1, 2, t)
        assert b[1][:2] == (0, 1) and b[1][2] == b[1][3] and b[0][3] > b[0][2] and b[2][3] > b[2][2]
        yield c
        # every read in one micro-window: more than one turn of the owner loop on one counter
        s = np.full(OWN_TURN + 1, 7 * E_STEP + 1, dtype=np.int64) + np.arange(OWN_TURN + 1) % E_STEP
        c = e_single("one-micro", cap, 2, (t * 2 * E_STEP, 40), cat(tri(0, np.sort(s), s.max() + 30)), E_STEP, "every read in micro-window 7")
        assert len(set(micro_of(c)[1].tolist())) == 1 and len(c.reads) > OWN_TURN
        yield c
        # starts below 1: dropped by the unsorted scanner's rule, counted in micro-window 0 by the sorted scanner's
        r = cat(tri(0, [-2000000000, -5, -5, 0, 0, 0], 40), tri(0, [-9, -3], [-1, 0]), fill(0, range(0, 2 * t, 3), E_STEP), tri(1, [-7, 0, 1], 50))
        c = e_single("below-one", cap, 2, (2 * t * E_STEP + 5, 40), r, E_STEP, "starts below 1 at the head of a class")
        assert (micro_of(c, True)[1] == 0).sum() >= (micro_of(c, False)[1] == 0).sum() + 8
        yield c
    # comb 2048: the owner pass takes it with blocks of 4096 windows; 2049: it declines and the general kernels serve
    for comb, want in ((WIN_MAX_COMB, 4096), (WIN_MAX_COMB + 1, 0)):
        assert own_tile(64, comb) == want and own_tile(None, comb) == want
        n_micro = comb + 99
        r = cat(fill(0, set(near([0, comb - 1, comb, 99, 100, n_micro - 1], 12, 0, n_micro)) | set(range(0, n_micro, 9)), 1), fill(1, range(0, 30, 2), 1))
        yield Case("E-comb%d" % comb, ordered(r), (n_micro, 30), 1, comb, "1", "comb %d: owner tile %d" % (comb, want))
    # the class of the largest length there is, step 2^20: the last block's end key lies beyond INT_MAX.  (For a block that is not the
    # last of its class the key is at most (nMicro - 1) * step + 1 <= class length: `endPos > INT_MAX` holds in a last block only.)
    comb = 65
    t = own_tile(64, comb)
    n_micro = MAX_LEN // E_TOP_STEP
    ms = set(near([0, n_micro - 1, n_micro - comb, n_micro - comb + 1] + [k * t for k in range(9)], 3, 0, n_micro)) | set(range(0, n_micro, 11))
    r = cat(fill(0, ms, E_TOP_STEP), at_positions(0, [n_micro * E_TOP_STEP, n_micro * E_TOP_STEP + 1, TOP - 1, TOP]), fill(1, range(70), E_TOP_STEP))
    c = Case("E-top-T%d" % t, ordered(r), (MAX_LEN, 70 * E_TOP_STEP), E_TOP_STEP, comb * E_TOP_STEP, "1", "the last block's end key lies beyond INT_MAX; reads at the top")
    b, _ = own_bounds(c.reads, c.class_len, c.step, c.size, t)
    last0 = [x for x in b if x[0] == 0][-1]
    assert t == 256 and last0[4] and not any(x[4] for x in b if x is not last0) and has_read_at(c, 0, TOP)
    yield c


# ---- F: the owner pass's order check -----------------------------------------------------------------------------------------------
F_COMB = 3
F_LEN = (4 * 64 + F_COMB - 1, F_COMB - 1, 200)          # step 1: 256 windows (four blocks of 64), none, 198
F_KINDS = ("start", "class")


@functools.lru_cache(maxsize=None)
def f_stream():
    """reads in order: about 20 per micro-window of class 0 (a block of 64 windows owns more than a turn of the owner loop), reads of a
    class without windows, of a class with windows, and trailing reads of an unknown class; many equal keys"""
    r = cat(fill(0, range(F_LEN[0]), 1, mult=8), at_positions(1, [1] * 3 + [2] * 3 + [5] * 3), fill(2, range(0, 200, 2), 1), at_positions(5, [3, 3, 4, 9, 9, 12]))
    assert in_order(r) and (np.diff(_i64(r)[:, 1])[np.diff(_i64(r)[:, 0]) == 0] == 0).any()
    r.setflags(write=False)
    return r


def f_places():
    """name -> index of the read that is made to sort before its predecessor"""
    r = f_stream()
    b64, n = own_bounds(r, F_LEN, 1, F_COMB, 64)
    own = [x[2] for x in b64] + [n]
    assert b64[1][:2] == (0, 1) and own[2] - own[1] > OWN_TURN + 64
    cls = _i64(r)[:, 0]
    first = {c: int(np.flatnonzero(cls == c)[0]) for c in (1, 2, 5)}
    tail = (own[2] + b64[1][3]) // 2                                                 # block 1 counts it, block 2 owns (and checks) it
    assert own[2] < tail < b64[1][3]
    places = {"read1": 1, "own-first": own[1], "own-second": own[1] + 1, "own-plus64": own[1] + 64, "own-plus1024": own[1] + OWN_TURN, "shared-tail": tail,
              "class-without-windows": first[1] + 4, "unknown-class": first[5] + 3}
    assert own[1] + OWN_TURN < own[2] and cls[first[1] + 4] == 1 and cls[first[5] + 3] == 5
    return places


def family_f():
    base = f_stream()
    yield Case("F-in-order", base.copy(), F_LEN, 1, F_COMB, "1", "the stream in order, equal keys included: no break")
    for place, i in f_places().items():
        for kind in F_KINDS:
            r = base.copy()
            if kind == "start":
                if r[i, 0] != r[i - 1, 0]:
                    continue
                r[i, 1] = r[i - 1, 1] - 1
                r[i, 2] = r[i, 1] + 35
            else:
                r[i - 1, 0] += 1
            q = _i64(r)
            key = q[:, 0] * (1 << 33) + (q[:, 1] + (1 << 31))
            assert np.flatnonzero(np.diff(key) < 0).tolist() == [i - 1], (place, kind)  # broken in exactly one place
            yield Case("F-%s-by-%s" % (place, kind), r, F_LEN, 1, F_COMB, "1", "the order breaks at read %d (%s) by %s" % (i, place, kind))


# ---- G: parts and buckets of the partition path ------------------------------------------------------------------------------------
G_COMB = (1, 2, 64, 65)
G_BASES = (BKT_MIN_PER, BINS64)   # a bucket is one part of 16384 micro-windows unweighted, of 15360 (16384 cut to whole parts) weighted


def g_n_micro(base, comb):
    return sorted({base - 1, base, base + 1, base + comb - 2, base + comb - 1, base + comb, 2 * base + 1})


def g_reads(cls, n_micro, comb, cuts):
    seams = [c for c in cuts if c <= n_micro + comb] + [0, n_micro - 1, n_micro - comb, n_micro - comb + 1]
    return fill(cls, near(seams, comb + 1, 0, n_micro + 3), 1)                        # (a few beyond the class's last micro-window)


def g_case(base, comb, n_micro):
    cuts = [k * b for b in G_BASES for k in (1, 2)]
    lens = (n_micro, 300 + comb, 90)                                                 # the second class has windows and no read at all
    r = cat(g_reads(0, n_micro, comb, cuts), fill(2, range(0, 90, 2), 1))
    return Case("G-base%d-comb%d-n%d" % (base, comb, n_micro), r, lens, 1, comb, "1", "cuts at multiples of %d (unweighted) and %d (weighted)" % G_BASES)


def g_aim(case, cuts, comb):
    cls, m = micro_of(case)
    have = set(m[cls == 0].tolist())
    n_micro = case.class_len[0]
    for cut in cuts:
        if cut < n_micro:
            want = [x for x in range(cut - comb, cut + comb + 1) if 0 <= x < n_micro]
            assert set(want) <= have, (case.name, cut)
            k = np.bincount(m[cls == 0], minlength=n_micro)[want]
            assert (np.diff(k) != 0).all(), (case.name, cut)                          # distinct counts on neighbouring micro-windows


def family_g():
    seen = set()
    for base in G_BASES:
        for comb in G_COMB:
            for n_micro in g_n_micro(base, comb):
                case = g_case(base, comb, n_micro)
                if case.name.split("-", 2)[2] in seen:
                    continue
                seen.add(case.name.split("-", 2)[2])
                g_aim(case, [k * b for b in G_BASES for k in (1, 2)], comb)
                cls = _i64(case.reads)[:, 0]
                assert not (cls == 1).any() and layout(case.class_len, 1, comb)[1][1] > 0
                yield case
                if comb >= FUSED_MAX_COMB and n_micro == base + comb - 1:
                    yield centred(case)


# ---- H: buckets of two and three parts, the last one short (the child process with GTX_SCAN_BUCKETS=1) -----------------------------
H_BASES = (2 * BINS32, 2 * BINS64, 3 * BINS64)


def h_per(n_micro, weighted):
    """the bucket width the case is built for (tests/test_scan_cases_cpu.py asks the library's rule for it)"""
    bins = BINS64 if weighted else BINS32
    return n_micro // bins * bins if n_micro > bins else max(n_micro, BKT_MIN_PER)


def family_h():
    seen = set()
    for base in H_BASES:
        for comb in G_COMB:
            for r in (0, 1, comb - 2, comb - 1, comb):
                n_micro = base + r
                if r < 0 or (comb, n_micro) in seen:
                    continue
                seen.add((comb, n_micro))
                cuts = sorted({k * b for b in (BINS32, BINS64) for k in range(1, 7) if k * b <= n_micro})
                case = Case("H-base%d-comb%d-r%d" % (base, comb, r), g_reads(0, n_micro, comb, cuts), (n_micro,), 1, comb, "1",
                            "one class of %d micro-windows: whole parts and a last bucket of %d" % (n_micro, r))
                g_aim(case, cuts, comb)
                weighted = base != 2 * BINS32                                        # the kind of call the case aims at; the other kind cuts it too
                per = h_per(n_micro, weighted)
                assert per == base and n_micro - per == r and per // (BINS64 if weighted else BINS32) == (3 if base == 3 * BINS64 else 2)
                yield case


GENERATORS = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f, "G": family_g, "H": family_h}
MAX_READS, MAX_MICRO = 70000, 1 << 17


@functools.lru_cache(maxsize=None)
def family(fam):
    """the cases of one family without weights (generated once per process; running a generator to its end checks the family's aim)"""
    out = list(GENERATORS[fam]())
    assert len({c.name for c in out}) == len(out)
    for c in out:
        assert c.size % c.step == 0 and len(c.reads) <= MAX_READS and int(layout(c.class_len, c.step, c.size)[0].sum()) <= MAX_MICRO, c.name
        c.reads.setflags(write=False)
    return out


def by_name(name):
    return next(c for c in family(name[0]) if c.name == name)


def shuffled(case):
    """the reads (and the permutation, for the weights) in no order"""
    p = np.random.default_rng(zlib.crc32(case.name.encode())).permutation(len(case.reads))
    return np.ascontiguousarray(case.reads[p]), p


@functools.lru_cache(maxsize=None)
def wanted(fam, sorted_rule=False):
    """brute() of every case of a family in every weight variant, computed once: {case name: {variant: windows}}"""
    out = {}
    for c in family(fam):
        ws = [weights_for(c.name, len(c.reads), v) for v in VARIANTS]
        res = brute_multi(c.reads, c.class_len, c.step, c.size, c.prep, ws, sorted_rule)
        for r in res:
            r.setflags(write=False)
        out[c.name] = dict(zip(VARIANTS, res))
    return out
