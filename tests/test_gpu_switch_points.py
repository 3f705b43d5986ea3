"""Every kernel-path switch the library takes by itself from the shape of a call, with cases on both sides of the threshold
(tests/switch_points.py; tests/test_switch_points_cpu.py keeps the table equal to the sources).  Each case is checked against what
the other tests check against -- the CPU oracle (oracle/orc.py), the oracle's `pairs` rows, oracle.restate's offsets and
test_gpu_signal.expected -- and asserts the quantity that decides its switch, so that it cannot drift off the switch point."""
import os

import numpy as np
import pytest

import gtx
import switch_points as sp
import test_gpu_join as tj
import test_gpu_offset as to
import test_gpu_signal as ts
from gtx import synth
from oracle import orc
from oracle.restate import regions, take, triples

pytestmark = pytest.mark.gpu

N_CLASSES = 24


def engine_with(**env):
    """a second context made under per-context knobs (read at gtx_create only)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return gtx.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def class_refs(rng, per_class, span=2_000_000):
    """per_class[c] valid regions of class c (50 to 2000 bases), sorted by (class, start)"""
    c = np.repeat(np.arange(len(per_class)), per_class)
    s = rng.integers(1, span, size=len(c))
    a = np.stack([c, s, s + rng.integers(49, 2000, size=len(c))], axis=1)
    return a[np.lexsort((a[:, 1], a[:, 0]))].astype(np.int32)


def class_reads(rng, n, n_classes=N_CLASSES, span=2_000_000, sort=True):
    c = rng.integers(0, n_classes, size=n)
    s = rng.integers(1, span, size=n)
    a = np.stack([c, s, s + rng.integers(49, 150, size=n)], axis=1)
    return (a[np.lexsort((a[:, 1], a[:, 0]))] if sort else a).astype(np.int32)


def spread(n_valid):
    return synth.apportion(n_valid, np.ones(N_CLASSES))


def device_counts(e, torch, reads, m, w=None):
    d_r = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    d_w = None if w is None else torch.from_numpy(w).cuda()
    hits = torch.full((max(m, 1),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.count_device(d_r.data_ptr(), len(reads), hits.data_ptr(), None if d_w is None else d_w.data_ptr())
    e.sync()
    info = e.last_info()
    return hits.cpu().numpy().view(np.uint64)[:m], info


# ---- rows 1-3: the finalize routes x tile sums kept or not x slot width ----

EDGE = [1023, 1023, 0] + [1] * (N_CLASSES - 3)       # class 1 starts at slot 1024; class 2 is empty, its one slot at 2048
LAYOUTS = {
    "tiles1": spread(sp.TILE - N_CLASSES),
    "tiles2": spread(sp.TILE - N_CLASSES + 1),
    "tiles512": spread(sp.CHAIN_MAX_TILES * sp.TILE - N_CLASSES),
    "tiles513": spread(sp.CHAIN_MAX_TILES * sp.TILE - N_CLASSES + 1),
    "class_edges": np.array(EDGE),
}
_want = {}
WANT_TILES = {"tiles1": 1, "tiles2": 2, "tiles512": sp.CHAIN_MAX_TILES, "tiles513": sp.CHAIN_MAX_TILES + 1, "class_edges": 3}


@pytest.fixture(scope="module")
def big_reads():
    rng = np.random.default_rng(2020)
    reads = class_reads(rng, sp.TILE_SUMS_MAX_READS)
    w = rng.integers(-3, 9, size=len(reads)).astype(np.int32)
    return reads, w


@pytest.mark.parametrize("n_reads", [sp.TILE_SUMS_MAX_READS - 1, sp.TILE_SUMS_MAX_READS], ids=["sums_kept", "sums_rebuilt"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_finalize_routes(engine, big_reads, layout, n_reads):
    """tiles <= CHAIN_MAX_TILES with the tile sums not kept: the chained one-launch finalize; above: tile_sums + finalize_scan;
    kept (< TILE_SUMS_MAX_READS reads in the launch): finalize_scan alone.  Through the host entry (64-bit slots), the device entry
    (32-bit slots) and the device entry with weights (64-bit)"""
    torch = pytest.importorskip("torch")
    per_class = LAYOUTS[layout]
    refs = class_refs(np.random.default_rng(len(layout) + int(per_class.sum())), per_class)
    assert sp.tiles(len(refs), N_CLASSES) == WANT_TILES[layout]
    if layout == "class_edges":
        first_slot = np.concatenate(([0], np.cumsum(per_class)[:-1])) + np.arange(N_CLASSES)
        assert first_slot[1] == sp.TILE and first_slot[2] == 2 * sp.TILE and per_class[2] == 0
    reads, w = big_reads[0][:n_reads], big_reads[1][:n_reads]
    assert len(reads) >= sp.TILE_SUMS_MAX_READS - 1 and len(reads) <= sp.TILE_SUMS_MAX_READS
    engine.set_refs(refs, N_CLASSES)
    if layout not in _want:                                                # the oracle over all reads, once per layout
        _want[layout] = (orc.count(refs, big_reads[0], algo=orc.BIN_INDEX), orc.count(refs, big_reads[0], big_reads[1], algo=orc.BIN_INDEX))
    want, want_w = _want[layout]
    if n_reads < len(big_reads[0]):                                        # ... less the reads left out (counts add up over reads)
        rest, rest_w = big_reads[0][n_reads:], big_reads[1][n_reads:]
        want, want_w = want - orc.count(refs, rest, algo=orc.BIN_INDEX), want_w - orc.count(refs, rest, rest_w, algo=orc.BIN_INDEX)
    # non-zero counts in the first and the last tile, and on both sides of the class edges
    assert want[:64].sum() > 0 and want[-64:].sum() > 0 and (want > 0).mean() > 0.9
    if layout == "class_edges":
        assert want[refs[:, 0] == 0][-1] > 0 and want[refs[:, 0] == 1][0] > 0 and want[refs[:, 0] == 3][0] > 0
    hits, info = engine.count(reads, None, gtx.READS_SORTED)
    np.testing.assert_array_equal(hits, want)
    assert info["n_no_class"] == 0
    got, info = device_counts(engine, torch, reads, len(refs))
    np.testing.assert_array_equal(got, want)
    got, info = device_counts(engine, torch, reads, len(refs), w)
    np.testing.assert_array_equal(got, want_w)


# ---- row 4: the all-boundaries-at-once walk (flip) at n_reads == FLIP_RATIO * n_valid ----

@pytest.mark.parametrize("extra", [0, 1], ids=["flip", "loop"])
def test_flip_kernel(engine, extra):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(64 + extra)
    refs = class_refs(rng, spread(4096))
    n = sp.FLIP_RATIO * len(refs) + extra
    assert n < sp.TILE_SUMS_MAX_READS
    reads = class_reads(rng, n)
    engine.set_refs(refs, N_CLASSES)
    want = orc.count(refs, reads, algo=orc.BIN_INDEX)
    assert (want > 0).mean() > 0.9
    hits, _ = engine.count(reads, None, gtx.READS_SORTED)                 # count_walk_kernel_flip / count_walk_kernel
    np.testing.assert_array_equal(hits, want)
    got, _ = device_counts(engine, torch, reads, len(refs))               # count_walk_kernel_flip_h32 / count_walk_kernel_h32
    np.testing.assert_array_equal(got, want)


# ---- row 5: reads in no order -- per-read search or the partition path at BUCKET_MIN_READS ----

@pytest.fixture(scope="module")
def shuffled():
    rng = np.random.default_rng(18)
    refs = synth.genome_intervals(30_000, 181, 50, 100_000)
    reads = synth.genome_intervals(sp.BUCKET_MIN_READS + 1, 182, 50, 300, sort=False)
    return refs, reads[rng.permutation(len(reads))]


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_unsorted_partition_path(engine, shuffled, delta):
    refs, all_reads = shuffled
    reads = np.ascontiguousarray(all_reads[:sp.BUCKET_MIN_READS + delta])
    assert len(reads) - sp.BUCKET_MIN_READS == delta
    engine.set_refs(refs, synth.n_classes())
    want = orc.count(refs, reads, algo=orc.BIN_INDEX)
    assert want.sum() > 10_000
    hits, _ = engine.count(reads, None, 0)
    np.testing.assert_array_equal(hits, want)
    cov, _ = engine.coverage(reads, None, gtx.READS_UNSORTED)
    want_c = orc.coverage(refs, reads, algo=orc.BIN_INDEX)
    assert want_c.sum() > 0
    np.testing.assert_array_equal(cov, want_c)
    win, _ = engine.scan(reads, synth.CHROM_LEN, 10_000, 10_000, flags=gtx.READS_UNSORTED)
    want_w, _ = orc.scan(reads, synth.CHROM_LEN, 10_000, 10_000)
    assert want_w.sum() > 0
    np.testing.assert_array_equal(win, want_w)


# ---- row 6: scan partition tables up to SCAN_BKT_MAX_CLASSES classes ----

@pytest.mark.parametrize("n_classes", [sp.SCAN_BKT_MAX_CLASSES, sp.SCAN_BKT_MAX_CLASSES + 1])
def test_scan_partition_tables(engine, n_classes):
    """shuffled reads over n_classes classes of 50 windows each: one bucket per class (SCAN_BKT_MIN_PER micro-windows or fewer),
    so the partition tables serve SCAN_BKT_MAX_CLASSES classes and the general kernels one more.  (The bucket-count limit needs
    more than ~6 * 10^7 micro-windows with at most SCAN_BKT_MAX_CLASSES classes -- the 2000-bucket target keeps nB below it
    otherwise -- so only the class limit is reachable at a test's size.)"""
    rng = np.random.default_rng(n_classes)
    step = 1000
    class_len = np.full(n_classes, 50 * step, dtype=np.int64)
    n_micro = class_len // step
    assert (n_micro <= sp.SCAN_BKT_MIN_PER).all() and n_micro.sum() <= sp.SCAN_BKT_MIN_PER * 2000
    n_buckets = n_classes                                                  # (one each)
    assert n_buckets <= sp.SCAN_BKT_MAX_BUCKETS
    n = sp.BUCKET_MIN_READS + 7
    c = rng.integers(0, n_classes, size=n)
    s = rng.integers(1, 50 * step - 200, size=n)
    reads = np.stack([c, s, s + rng.integers(0, 150, size=n)], axis=1).astype(np.int32)
    assert reads[:, 0].max() == n_classes - 1
    win, _ = engine.scan(reads, class_len, step, step, flags=gtx.READS_UNSORTED)
    want, off = orc.scan(reads, class_len, step, step)
    assert (want[off[-1]:] > 0).any() and (want[:off[1]] > 0).any()
    np.testing.assert_array_equal(win, want)
    w = rng.integers(0, 5, size=n).astype(np.int32)
    win, _ = engine.scan(reads, class_len, step, step, weights=w, flags=gtx.READS_UNSORTED)
    np.testing.assert_array_equal(win, orc.scan(reads, class_len, step, step, weights=w)[0])


# ---- row 7: host batches of a context made with a small GTX_BATCH_READS ----

BATCH = 1000


@pytest.fixture(scope="module")
def batch_engine():
    e = engine_with(GTX_BATCH_READS=BATCH)
    yield e
    e.close()


@pytest.mark.parametrize("n", [5 * BATCH - 1, 5 * BATCH, 5 * BATCH + 1])
def test_host_batches(batch_engine, tmp_path, n):
    e = batch_engine
    rng = np.random.default_rng(n)
    assert abs(n - 5 * BATCH) <= 1
    refs = synth.genome_intervals(3000, 71, 50, 200_000)
    reads = synth.genome_intervals(n, 72, 50, 300)
    e.set_refs(refs, synth.n_classes())
    want = orc.count(refs, reads, algo=orc.BIN_INDEX)
    assert want.sum() > 0
    hits, info = e.count(reads, None, gtx.READS_SORTED | gtx.CHECK_SORTED)
    np.testing.assert_array_equal(hits, want)
    assert info["first_unsorted"] == -1
    cov, _ = e.coverage(reads)
    np.testing.assert_array_equal(cov, orc.coverage(refs, reads, algo=orc.BIN_INDEX))
    # join: the oracle's pairs over BED files of the same regions
    jr, jq = regions(rng, 2000, 300_000, 1, 3000), regions(rng, n, 300_000, 1, 300)
    want_j, off, pairs, _ = tj.run(e, tmp_path, jr, jq)
    assert len(off) == n + 1 and len(want_j) > 1000
    assert tj.join_rows(off, pairs) == want_j
    # signal bins
    regs = ts.make_refs(rng, 300, 300_000)
    reads_s = ts.make_reads(rng, n, 300_000)
    reads_s.sort(key=lambda r: (r[0], r[1][0][0]))
    strands = [bool(rng.integers(0, 2)) for _ in reads_s]
    w = rng.integers(-4, 12, n).astype(np.int64)
    ts.upload(e, regs, False)
    e.set_signal_bins(-5000.0, 5000.0, 100)
    tri, _, _ = ts.read_arrays(reads_s, strands, False)
    want_s, _, _ = ts.expected(regs, reads_s, strands, w, -5000.0, 5000.0, 100, False, None, False)
    got, inv, info = e.signal_bins(tri, w, 0)
    assert inv == -1 and info["n_binned"] > 0 and np.array_equal(got, want_s)


# ---- rows 8-10: the join's segment sort, offset scan and chunk cut ----

def clusters(sizes, strand=0, long_every=3, seed=8):
    """references in clusters, one per size, and one query per cluster that overlaps exactly `size` of them.  Every third region
    is long (100 k - 400 k bases), so the bin index's order of a segment (level first) is not its start order"""
    rng = np.random.default_rng(seed)
    s, e, qs, qe = [], [], [], []
    for i, k in enumerate(sizes):
        x = (i + 1) << 20
        for j in range(k):
            s.append(x + j); e.append(x + j + (int(rng.integers(100_000, 400_000)) if j % long_every == 0 else int(rng.integers(0, 60))))
        qs.append(x if k else x - 5000); qe.append(x + max(k, 1) - 1 if k else x - 4000)
    def make(s, e, st):
        s, e = np.array(s, dtype=np.int64), np.array(e, dtype=np.int64)
        n = len(s)
        r = dict(chrom=np.zeros(n, dtype=np.int64), strand=np.full(n, st, dtype=np.int64), s=s, e=e,
                 first=np.arange(n + 1, dtype=np.int64), blocks=np.stack([s, e], axis=1))
        return take(r, np.lexsort((r["s"], r["chrom"])))
    return make(s, e, strand), make(qs, qe, 0)


SEG_SIZES = [0, 1, 2, sp.JOIN_SMALL_SEG, sp.JOIN_SMALL_SEG + 1, sp.JOIN_LDS_SEG - 1, sp.JOIN_LDS_SEG, sp.JOIN_LDS_SEG + 1,
             2 * sp.JOIN_LDS_SEG, 2 * sp.JOIN_LDS_SEG + 1, 3 * sp.JOIN_LDS_SEG + 1]


@pytest.mark.parametrize("sorted_", [False, True], ids=["bin_keys", "ordinal_keys"])
def test_join_segment_sort(engine, tmp_path, sorted_):
    torch = pytest.importorskip("torch")
    refs, reads = clusters(SEG_SIZES)
    want, off, pairs, info = tj.run(engine, tmp_path, refs, reads, sorted_=sorted_)
    assert list(np.diff(off)) == SEG_SIZES
    assert tj.join_rows(off, pairs) == want
    if not sorted_:                                                        # the oracle's order is not the start order: the sort works
        for i, k in enumerate(SEG_SIZES):
            seg = [int(x.split("\tr")[1]) for x in want if x.startswith("%d\t" % (i + 1))]
            assert len(seg) == k and (k < 2 or seg != sorted(seg))
    d_reads = torch.from_numpy(triples(reads, True)).cuda()
    d_off = torch.zeros(len(off), dtype=torch.int64, device="cuda")
    d_pairs = torch.zeros(int(off[-1]), dtype=torch.int32, device="cuda")
    total, done, _ = engine.join_device(d_reads.data_ptr(), len(off) - 1, d_off.data_ptr(), d_pairs.data_ptr(), int(off[-1]),
                                        gtx.ZERO_LENGTH_OK if sorted_ else 0)
    assert total == off[-1] and done == len(off) - 1
    assert tj.join_rows(d_off.cpu().numpy(), d_pairs.cpu().numpy()) == want


def test_join_scan_partials(engine, tmp_path):
    """the one-block scan of the per-tile partials: one partial per lane at 256 * 2048 - 1 queries (n + 1 offsets), two from one more"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(9)
    n_one = sp.JOIN_SCAN_THREADS * sp.JOIN_SCAN_TILE - 1
    ns = [n_one, n_one + 1, n_one + 2]
    assert [sp.join_scan_per(n) for n in ns] == [1, 2, 2]
    refs, reads = regions(rng, 1500, 2_000_000, 1, 3000), regions(rng, ns[-1], 2_000_000, 1, 200)
    want, off, pairs, _ = tj.run(engine, tmp_path, refs, reads)
    assert tj.join_rows(off, pairs) == want
    d_reads = torch.from_numpy(triples(reads, True)).cuda()
    for n in ns:
        k = int(off[n])
        assert k > 100_000
        d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_pairs = torch.zeros(max(k, 1), dtype=torch.int32, device="cuda")
        total, done, _ = engine.join_device(d_reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), k)
        assert total == k and done == n
        assert np.array_equal(d_off.cpu().numpy(), off[:n + 1])
        assert tj.join_rows(d_off.cpu().numpy(), d_pairs.cpu().numpy()[:k]) == want[:k]


def test_join_buffer_cut(engine, tmp_path):
    """a join buffer and a capacity exactly at a segment's end, one pair short of it and one pair past it"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(10)
    refs, reads = regions(rng, 2000, 300_000, 1, 4000), regions(rng, 12_000, 300_000, 1, 3000)
    want, off, pairs, _ = tj.run(engine, tmp_path, refs, reads)
    full = [int(x.split("\tr")[1]) for x in want]
    seg = np.diff(off)
    q = int(np.flatnonzero((seg[:-1] > 1) & (seg[1:] > 1) & (off[1:-1] > 1000))[0]) + 1      # segments on both sides of off[q]
    end = int(off[q])
    assert off[q] - off[q - 1] > 1 and off[q + 1] - off[q] > 1
    d_reads = torch.from_numpy(triples(reads, True)).cuda()
    for b in (end - 1, end, end + 1):
        engine.set_join_buffer(b)
        o, p, _ = engine.join(triples(reads, True))
        assert np.array_equal(o, off) and list(p) == full
        o, p, _ = engine.join(triples(reads, True), capacity=b)
        assert np.array_equal(o, off) and list(p) == full[:b]
        d_off = torch.zeros(len(off), dtype=torch.int64, device="cuda")
        d_pairs = torch.zeros(b, dtype=torch.int32, device="cuda")
        total, done, _ = engine.join_device(d_reads.data_ptr(), len(off) - 1, d_off.data_ptr(), d_pairs.data_ptr(), b)
        assert total == off[-1] and done == (q if b == end else (q - 1 if b < end else q))
        assert off[done] <= b < off[done + 1]
        assert list(d_pairs.cpu().numpy()[:off[done]]) == full[:off[done]]
    engine.set_join_buffer(1 << 26)


# ---- row 11: pair offsets, one lane or one block per segment ----

OFF_SIZES = [sp.OFF_SMALL_SEG, sp.OFF_SMALL_SEG + 1, 2 * sp.OFF_SMALL_SEG, 2 * sp.OFF_SMALL_SEG + 1]


@pytest.mark.parametrize("op", ["5p", "3p"])
def test_pair_offset_segments(engine, tmp_path, op):
    refs, tests = clusters(OFF_SIZES, strand=1)
    assert (refs["strand"] == 1).all()
    rows, want, (off, pairs, eoff, ent, inv, _) = to.run(engine, tmp_path, refs, tests, op)
    assert list(np.diff(off)) == OFF_SIZES
    assert to.got_rows(off, pairs) == rows
    assert to.got_entries(eoff, ent) == want and len(ent) == sum(OFF_SIZES)
    assert inv == -1


@pytest.mark.parametrize("target", [sp.JOIN_SCAN_TILE - 1, sp.JOIN_SCAN_TILE, sp.JOIN_SCAN_TILE + 1])
def test_pair_offset_entry_scan(engine, tmp_path, target):
    """--skip-ref-gaps: the entry counts of one chunk's pairs (pairs + 1 values) are scanned in tiles of JOIN_SCAN_TILE"""
    rng = np.random.default_rng(11)
    refs = to.regions(rng, 600, 300_000, 1, 3000, multi=0.6)
    tests = to.concat(to.regions(rng, 1500, 300_000, 1, 200, multi=0.3), to.inside(rng, refs, 1500))
    tests = take(tests, np.lexsort((tests["s"], tests["chrom"])))
    rows, _, (off, _, _, _, _, _) = to.run(engine, tmp_path, refs, tests, "5p", skip=True)
    seg = np.diff(off)
    keep, tot = [], 0                                                      # queries (in order) whose pairs add up to target
    for i, k in enumerate(seg):
        if tot + k <= target:
            keep.append(i); tot += int(k)
    assert tot == target
    sub = take(tests, np.array(keep))
    rows, want, (off, pairs, eoff, ent, inv, _) = to.run(engine, tmp_path, refs, sub, "5p", skip=True)
    assert len(rows) == target and off[-1] == target
    assert to.got_rows(off, pairs) == rows and to.got_entries(eoff, ent) == want
    assert sum(len(x) > 1 for x in want) > 0 and len(ent) > 0 and inv == -1


# ---- row 12: signal bins, the profile row in LDS up to SIGNAL_LDS_BINS ----

@pytest.fixture(scope="module")
def signal_set():
    rng = np.random.default_rng(12)
    regs = ts.make_refs(rng, 240, 400_000)
    reads = ts.make_reads(rng, 24_000, 400_000)
    strands = [bool(rng.integers(0, 2)) for _ in reads]
    w = rng.integers(-5, 12, len(reads)).astype(np.int64)
    return regs, reads, strands, w


@pytest.mark.parametrize("per_ref", [False, True], ids=["profile", "heatmap"])
@pytest.mark.parametrize("n_bins", [1, sp.SIGNAL_LDS_BINS - 1, sp.SIGNAL_LDS_BINS, sp.SIGNAL_LDS_BINS + 1])
def test_signal_bins_lds_limit(engine, signal_set, n_bins, per_ref):
    regs, reads, strands, w = signal_set
    assert n_bins in (1, sp.SIGNAL_LDS_BINS - 1, sp.SIGNAL_LDS_BINS, sp.SIGNAL_LDS_BINS + 1)
    ts.upload(engine, regs, False)
    engine.set_signal_bins(-5000.0, 5000.0, n_bins)
    tri, _, _ = ts.read_arrays(reads, strands, False)
    want, winv, wdrop = ts.expected(regs, reads, strands, w, -5000.0, 5000.0, n_bins, per_ref, None, False)
    got, inv, info = engine.signal_bins(tri, w, gtx.SIGNAL_PER_REF if per_ref else 0)
    assert inv == winv == -1 and info["n_dropped"] == wdrop == 0
    assert info["n_binned"] > 1000 and (w < 0).any() and (want != 0).any()
    flat = want.reshape(-1, n_bins).sum(axis=0)
    assert flat[:max(1, n_bins // 8)].any() and flat[-max(1, n_bins // 8):].any()   # both ends of the row
    assert np.array_equal(got, want)
