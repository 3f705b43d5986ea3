"""Link on the device (gtx_link / gtx_link_device, csrc/gtx_link.hip) against the restatement of the reference's loop
(tests/link_restate.py: RunGlobalLink, genomic_intervals.cpp:4605-4644, on packed triples)."""
import numpy as np
import pytest

import gtx
import link_restate

pytestmark = pytest.mark.gpu

T = gtx.LINK_TILE
FOLDS = {"sum": gtx.LINK_SUM, "min": gtx.LINK_MIN, "max": gtx.LINK_MAX}


@pytest.fixture(scope="module")
def eng():
    e = gtx.Engine(0)
    yield e
    e.close()


def check(eng, tri, d=0, values=None, fold=None):
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    wh, wc, ws, wv, wu = link_restate.link_packed(tri, d, values, fold)
    h, c, s, v, info = eng.link(tri, values, d, FOLDS[fold] if fold else 0)
    assert info == {"n_groups": len(wh), "first_unsorted": wu}
    np.testing.assert_array_equal(h, wh)
    np.testing.assert_array_equal(c, wc)
    np.testing.assert_array_equal(s, ws)
    if fold:
        np.testing.assert_array_equal(v, wv)
    else:
        assert v is None
    return len(wh)


def sorted_regions(seed, n, n_classes, span, lmin=1, lmax=60):
    """n regions in (class, start) order; lengths from lmin (may be <= 0: zero-length and inverted regions) to lmax"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, n_classes, size=n)
    start = rng.integers(1, span + 1, size=n)
    order = np.lexsort((start, cls))
    cls, start = cls[order], start[order]
    stop = start + rng.integers(lmin, lmax + 1, size=n) - 1
    return np.stack([cls, start, stop], axis=1).astype(np.int32)


def test_tile_constant_is_the_headers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gtx.h")).read()
    assert int(re.search(r"#define GTX_LINK_TILE (\d+)", src).group(1)) == T
    for name, val in FOLDS.items():
        assert int(re.search(r"#define GTX_LINK_%s (\d+)u" % name.upper(), src).group(1)) == val


def test_empty_one_two(eng):
    assert check(eng, np.zeros((0, 3))) == 0
    assert check(eng, [[3, 5, 9]]) == 1
    assert check(eng, [[3, 5, 9], [3, 9, 12]]) == 1
    assert check(eng, [[3, 5, 9], [3, 10, 12]]) == 2          # adjacent: not joined at d = 0
    assert check(eng, [[3, 5, 9], [3, 10, 12]], d=1) == 1
    assert check(eng, [[3, 5, 9], [4, 6, 12]]) == 2           # another class
    assert check(eng, [[3, 5, 9]], values=[7], fold="sum") == 1


SIZES = [63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_wave_the_block_and_the_tile(eng, n):
    one = np.stack([np.zeros(n), np.arange(n) * 5 + 1, np.arange(n) * 5 + 10], axis=1)            # everything overlaps its neighbour
    assert check(eng, one) == 1
    none = np.stack([np.zeros(n), np.arange(n) * 20 + 1, np.arange(n) * 20 + 10], axis=1)         # nothing does
    assert check(eng, none) == n
    vals = np.random.default_rng(n).integers(-2**40, 2**40, size=n)
    assert check(eng, one, values=vals, fold="sum") == 1
    assert check(eng, none, values=vals, fold="min") == n
    tri = sorted_regions(n, n, 3, 12 * n)
    for fold in (None, "sum", "min", "max"):
        assert 1 < check(eng, tri, values=vals if fold else None, fold=fold) < n


def test_a_first_region_that_contains_every_other_over_more_than_two_tiles(eng):
    n = 2 * T + 300
    tri = np.stack([np.zeros(n), np.arange(n) * 100 + 1, np.arange(n) * 100 + 10], axis=1).astype(np.int64)
    tri[0] = [0, 1, 100 * n + 50]                      # its stop is the maximum that every later tile needs
    assert check(eng, tri) == 1
    assert check(eng, tri, values=np.arange(n), fold="max") == 1
    tri[0, 2] = 100 * (T + 7) + 5                      # ... up to the eighth region of the second tile
    assert check(eng, tri) == n - (T + 7)
    tri[0, 0] = -1                                     # a class of its own: nothing is carried
    assert check(eng, tri) == n


@pytest.mark.parametrize("at", [T, T - 1, T + 1, 2 * T, 64, 512])
def test_a_class_change_on_and_beside_a_tile_boundary(eng, at):
    n = 2 * T + 10
    tri = np.stack([np.zeros(n), np.arange(n) + 1, np.arange(n) + 2], axis=1).astype(np.int64)      # overlapping chain
    tri[at:, 0] = 1
    tri[at:, 1] -= at                                   # the new class starts below the old one's maximum
    tri[at:, 2] -= at
    assert check(eng, tri) == 2
    assert check(eng, tri, values=np.arange(n) - 5, fold="sum") == 2


@pytest.mark.parametrize("d", [0, 1, -1, -5, 1000, 2**31])
def test_max_difference(eng, d):
    tri = sorted_regions(5, 3 * T + 17, 4, 40 * T)
    g = check(eng, tri, d)
    assert (g == 4) if d == 2**31 else (4 <= g <= len(tri))


def test_coordinates_where_32_bits_wrap(eng):
    big = 2**31 - 3
    tri = [[0, -big, -big + 5], [0, big, big]]         # START - new_stop = 2^32 - 11
    assert check(eng, tri, d=2**31) == 2               # a 32-bit difference is -11 and would join
    assert check(eng, tri, d=2**32 - 11) == 1
    assert check(eng, tri, d=2**32 - 12) == 2
    tri = [[0, -big, big], [0, -big + 1, -big + 1]]    # START - new_stop = -(2^32 - 7)
    assert check(eng, tri, d=-(2**31)) == 1
    assert check(eng, tri, d=-(2**32 - 7)) == 1
    assert check(eng, tri, d=-(2**32 - 6)) == 2


@pytest.mark.parametrize("d", [0, -1, -5, 7])
def test_ties_nesting_zero_length_and_inverted_regions(eng, d):
    """where the class prefix maximum is not the group's: a closed group may hold the larger stop"""
    tri = sorted_regions(17 + d, 2 * T + 77, 3, 3 * T, lmin=-4, lmax=12)          # ~2 regions per start
    vals = np.random.default_rng(3).integers(-1000, 1000, size=len(tri))
    wh, _, ws, _, _ = link_restate.link_packed(tri, d)
    if d < 0:
        last = np.concatenate((wh[1:], [len(tri)])).astype(np.int64) - 1
        pm = np.array([tri[:b + 1][tri[:b + 1, 0] == tri[b, 0]][:, 2].max() for b in last])
        assert (pm != ws).any()                                                    # the shortcut would be caught here
    check(eng, tri, d)
    check(eng, tri, d, vals, "sum")


def test_strand_folded_into_the_class(eng):
    rng = np.random.default_rng(8)
    n = T + 100
    chrom, strand = rng.integers(0, 3, size=n), rng.integers(0, 2, size=n)
    start = rng.integers(1, 4000, size=n)
    stop = start + rng.integers(1, 30, size=n)
    by_strand = np.lexsort((start, strand, chrom))
    with_s = np.stack([chrom * 2 + strand, start, stop], axis=1)[by_strand]
    by_pos = np.lexsort((start, chrom))
    without = np.stack([chrom, start, stop], axis=1)[by_pos]
    assert check(eng, with_s) > check(eng, without)


@pytest.fixture(scope="module")
def big_sets():
    """200 000 regions over 24 classes at three densities, and the restatement's answer for each, computed once"""
    sets = {}
    for name, span in (("dense", 40_000), ("medium", 400_000), ("sparse", 20_000_000)):
        tri = sorted_regions(len(name), 200_000, 24, span, 1, 60)
        vals = np.random.default_rng(span).integers(-2**40, 2**40, size=len(tri))
        sets[name] = (tri, vals, {f: link_restate.link_packed(tri, 0, vals, f) for f in (None, "sum", "min", "max")})
    return sets


@pytest.mark.parametrize("fold", [None, "sum", "min", "max"])
@pytest.mark.parametrize("name", ["dense", "medium", "sparse"])
def test_200k_random_regions(eng, big_sets, name, fold):
    tri, vals, want = big_sets[name]
    wh, wc, ws, wv, wu = want[fold]
    h, c, s, v, info = eng.link(tri, vals if fold else None, 0, FOLDS[fold] if fold else 0)
    assert info == {"n_groups": len(wh), "first_unsorted": -1}
    np.testing.assert_array_equal(h, wh)
    np.testing.assert_array_equal(c, wc)
    np.testing.assert_array_equal(s, ws)
    if fold:
        np.testing.assert_array_equal(v, wv)
    assert {"dense": len(wh) < 5000, "medium": 20_000 < len(wh) < 150_000, "sparse": len(wh) > 150_000}[name]


@pytest.mark.parametrize("at", [1, T + 700, T, 2 * T, 2 * T + 63, 2 * T + 64])
@pytest.mark.parametrize("how", ["start", "class"])
def test_an_unsorted_region(eng, at, how):
    tri = sorted_regions(at, 3 * T + 5, 2, 30 * T).astype(np.int64)
    if how == "start":
        tri[at, 0] = tri[at - 1, 0]
        tri[at, 1] = tri[at - 1, 1] - 1
    else:
        tri[at, 0] = tri[at - 1, 0] - 1
    wh, _, _, _, wu = link_restate.link_packed(tri, 0)
    assert wu == at and (len(wh) == 0 or wh[-1] < at)
    check(eng, tri)
    check(eng, tri, 0, np.arange(len(tri)), "sum")
    tri[at + 1:, 1] = 0                                # whatever follows the first unsorted region plays no part
    check(eng, tri)


def test_device_call_on_torch_tensors(eng):
    import torch
    tri = sorted_regions(2, 3 * T + 11, 5, 20 * T)
    vals = np.random.default_rng(4).integers(-10**9, 10**9, size=len(tri))
    wh, wc, ws, wv, wu = link_restate.link_packed(tri, 3, vals, "sum")
    n = len(tri)
    d_tri = torch.from_numpy(tri).cuda()
    d_vals = torch.from_numpy(vals).cuda()
    d_h = torch.zeros(n, dtype=torch.int32, device="cuda"); d_c = torch.zeros_like(d_h); d_s = torch.zeros_like(d_h)
    d_v = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    info = eng.link_device(d_tri.data_ptr(), n, d_h.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), d_vals.data_ptr(), d_v.data_ptr(), 3, gtx.LINK_SUM)
    eng.sync()
    assert info.as_dict() == {"n_groups": len(wh), "first_unsorted": wu}
    g = len(wh)
    np.testing.assert_array_equal(d_h.cpu().numpy()[:g].view(np.uint32), wh)
    np.testing.assert_array_equal(d_c.cpu().numpy()[:g].view(np.uint32), wc)
    np.testing.assert_array_equal(d_s.cpu().numpy()[:g], ws)
    np.testing.assert_array_equal(d_v.cpu().numpy()[:g], wv)
    # without a fold: no values needed
    info = eng.link_device(d_tri.data_ptr(), n, d_h.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), None, None, 3, 0)
    eng.sync()
    assert info.as_dict() == {"n_groups": len(wh), "first_unsorted": wu}
    np.testing.assert_array_equal(d_s.cpu().numpy()[:g], ws)


def test_two_device_calls_and_one_sync(eng):
    """each call's info reaches its own struct, whether the next call or the sync is what waits for it"""
    import torch
    a = sorted_regions(21, 2 * T + 5, 3, 30 * T)
    b = sorted_regions(22, T + 9, 2, 4 * T).astype(np.int64)
    b[T // 2, 1] = b[T // 2 - 1, 1] - 1; b[T // 2, 0] = b[T // 2 - 1, 0]          # an unsorted region in the second input
    b = b.astype(np.int32)
    want_a, want_b = link_restate.link_packed(a, 0), link_restate.link_packed(b, 2)
    bufs = []
    for tri in (a, b):
        n = len(tri)
        bufs.append((torch.from_numpy(tri).cuda(), [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]))
    torch.cuda.synchronize()
    (da, oa), (db, ob) = bufs
    ia = eng.link_device(da.data_ptr(), len(a), oa[0].data_ptr(), oa[1].data_ptr(), oa[2].data_ptr(), None, None, 0, 0)
    ib = eng.link_device(db.data_ptr(), len(b), ob[0].data_ptr(), ob[1].data_ptr(), ob[2].data_ptr(), None, None, 2, 0)
    eng.sync()
    assert ia.as_dict() == {"n_groups": len(want_a[0]), "first_unsorted": -1} and len(want_a[0]) > 1
    assert ib.as_dict() == {"n_groups": len(want_b[0]), "first_unsorted": T // 2}
    np.testing.assert_array_equal(oa[2].cpu().numpy()[:len(want_a[0])], want_a[2])
    np.testing.assert_array_equal(ob[2].cpu().numpy()[:len(want_b[0])], want_b[2])
    del ia, ib                                                                   # dropped before the next sync: the binding keeps them alive
    eng.link_device(da.data_ptr(), len(a), oa[0].data_ptr(), oa[1].data_ptr(), oa[2].data_ptr(), None, None, 0, 0)
    eng.sync()


def test_bad_arguments(eng):
    tri = sorted_regions(1, 10, 1, 100)
    vals = np.arange(10)
    with pytest.raises(gtx.GtxError):
        eng.link(tri, vals, 0, gtx.LINK_SUM | gtx.LINK_MAX)          # two folds
    with pytest.raises(gtx.GtxError):
        eng.link(tri, None, 0, gtx.LINK_SUM)                         # a fold without values
    with pytest.raises(gtx.GtxError):
        eng.link(tri, vals, 0, 8)                                    # no such flag
    check(eng, tri)                                                  # the context is still good


@pytest.fixture(scope="module")
def many_tiles():
    """1025 T + 1 regions over 24 classes at a density where the tiles differ in their number of heads"""
    n = 1025 * T + 1
    return sorted_regions(77, n, 24, 2 * n, 1, 60).astype(np.int64)


@pytest.mark.parametrize("unsorted", [False, True], ids=["sorted", "unsorted-in-the-last-tile"])
def test_more_tiles_than_threads_in_the_heads_prefix(eng, many_tiles, unsorted):
    """The one-block exclusive sum of the tiles' heads (block_exclusive_sum, csrc/gtx_compact.h) with two tiles to a thread and the
    upper half of its threads without one.  With the last region unsorted, the groups that count are read behind that sum at a
    base that is not zero."""
    tri = many_tiles.copy()
    if unsorted:
        tri[-1, 0] = tri[-2, 0]
        tri[-1, 1] = tri[-2, 1] - 1
    groups = check(eng, tri)
    assert len(tri) // 8 < groups < len(tri) - len(tri) // 8
    heads = np.bincount(eng.link(tri)[0] // T, minlength=1026)
    assert len(set(heads[:1025].tolist())) > 8                                   # the tiles' counts vary
