"""The neighbour passes on the device (gtx_adjacent / gtx_gaps and their _device entries, csrc/gtx_adjacent.hip) against the
restatement of the reference's loops on packed triples (tests/adjacent_restate.py: RunGlobalTest, RunGlobalCalcDistances and
RunGlobalInvert, genomic_intervals.cpp:4755-4778, :4523-4542, :4576-4600), bit for bit."""
import itertools
import os
import re

import numpy as np
import pytest

import gtx
import adjacent_restate as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gtx.h")).read()
T = int(re.search(r"#define GTX_ADJACENT_TILE (\d+)", HEADER).group(1))
BIG = 2**31 - 3


@pytest.fixture(scope="module")
def eng():
    e = gtx.Engine(0)
    yield e
    e.close()


def check_pairs(eng, tri, minus=None, op1=0, op2=0):
    """gtx_adjacent with and without distances against the packed loop; returns (first_unsorted, inclusions, overlaps)"""
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    wd, wu, wi, wo = ar.adjacent_packed(tri, minus, op1, op2)
    want = {"first_unsorted": wu, "n_inclusions": wi, "n_overlaps": wo}
    dist, info = eng.adjacent(tri, minus, op1, op2, want_dist=True)
    assert info == want
    np.testing.assert_array_equal(dist, wd)
    none, info = eng.adjacent(tri, minus, op1, op2)
    assert none is None and info == want
    return wu, wi, wo


def check_gaps(eng, tri, bounds, capacity=None):
    """gtx_gaps against the packed loop; returns (number of gaps, first_bad, bad_kind)"""
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    wo, ws, we, wb, wk = ar.gaps_packed(tri, bounds)
    o, s, e, info = eng.gaps(tri, bounds, capacity)
    assert info == {"n_gaps": len(wo), "first_bad": wb, "bad_kind": wk}
    got = len(wo) if capacity is None else min(len(wo), capacity)
    np.testing.assert_array_equal(o, wo[:got])
    np.testing.assert_array_equal(s, ws[:got])
    np.testing.assert_array_equal(e, we[:got])
    return len(wo), wb, wk


def sorted_regions(seed, n, n_classes, span, lmin=1, lmax=60):
    """n regions in (class, start) order; lengths from lmin (may be <= 0: zero-length and inverted regions) to lmax"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, n_classes, size=n)
    start = rng.integers(1, span + 1, size=n)
    order = np.lexsort((start, cls))
    cls, start = cls[order], start[order]
    stop = start + rng.integers(lmin, lmax + 1, size=n) - 1
    return np.stack([cls, start, stop], axis=1).astype(np.int32)


def test_constants_are_the_headers():
    assert T == gtx.ADJACENT_TILE
    for word, name in (("1", "START"), ("2", "STOP"), ("5p", "5P"), ("3p", "3P")):
        assert int(re.search(r"#define GTX_POINT_%s\s+(\d+)" % name, HEADER).group(1)) == gtx.POINTS[word] == ar.POINTS[word]


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_wave_the_block_and_the_tile(eng, n):
    tri = sorted_regions(n + 1, n, 3, 25 * max(n, 1))
    minus = np.random.default_rng(n).integers(0, 2, size=n).astype(np.uint8)
    u, i, o = check_pairs(eng, tri, minus, gtx.POINTS["5p"], gtx.POINTS["2"])
    assert u == -1 and (n < 255 or (i > 0 and o > 0))
    g, bad, _ = check_gaps(eng, tri, [25 * max(n, 1) + 100] * 3)
    assert bad == -1 and (n < 63 or g > n // 4)
    chain = np.stack([np.zeros(n), np.arange(n) * 5 + 1, np.arange(n) * 5 + 10], axis=1)          # everything overlaps its neighbour
    assert check_pairs(eng, chain) == (-1, 0, max(n - 1, 0))
    assert check_gaps(eng, chain, [5 * n + 5])[0] == 0                       # no gap at all: it fills [1, size]
    apart = np.stack([np.zeros(n), np.arange(n) * 20 + 5, np.arange(n) * 20 + 10], axis=1)         # nothing does
    assert check_pairs(eng, apart) == (-1, 0, 0)
    assert check_gaps(eng, apart, [20 * n + 100])[0] == (n + 1 if n else 0)


@pytest.mark.parametrize("at", [T - 1, T, T + 1, 2 * T, 64, 512])
def test_a_class_change_on_and_beside_a_tile_boundary(eng, at):
    n = 2 * T + 10
    tri = np.stack([np.zeros(n), 3 * np.arange(n) + 2, 3 * np.arange(n) + 3], axis=1).astype(np.int64)   # one free base between neighbours
    tri[at:, 0] = 1
    tri[at:, 1] -= 3 * at                                # the new class starts at 2 again, below its predecessor
    tri[at:, 2] -= 3 * at
    assert check_pairs(eng, tri, None, 1, 0) == (-1, 0, 0)
    dist, _ = eng.adjacent(tri.astype(np.int32), None, 1, 0, want_dist=True)
    assert dist[at] == ar.NO_DISTANCE and dist[at - 1] == 2 and dist[at + 1] == 2
    # leading + between gaps of both runs, and a trailing gap for each
    assert check_gaps(eng, tri, [3 * n + 50, 3 * n + 50]) == (n + 2, -1, 0)
    assert check_gaps(eng, tri, [3 * at, 3 * n + 50]) == (n + 1, -1, 0)      # the first run ends on its bound: no trailing gap


@pytest.mark.parametrize("at", [1, T - 1, T, T + 1, 2 * T + 63, 2 * T + 64])
@pytest.mark.parametrize("how", ["start", "class", "no_bound", "class_out_of_range"])
def test_the_first_bad_region(eng, at, how):
    tri = sorted_regions(at, 3 * T + 5, 2, 30 * T).astype(np.int64)
    bounds = [30 * T + 100, 30 * T + 100]
    if how == "start":
        tri[at, 0] = tri[at - 1, 0]
        tri[at, 1] = tri[at - 1, 1] - 1
    elif how == "class":
        tri[at, 0] = tri[at - 1, 0] - 1                  # before its predecessor for gtx_adjacent; the head of a run for gtx_gaps
    else:
        tri[at:, 0] += 5                                 # classes 5 and 6 from here on: a run head without a bound
        bounds = bounds + [-1] * 5 if how == "no_bound" else bounds
    u, _, _ = check_pairs(eng, tri)
    assert u == (at if how in ("start", "class") else -1)
    g, bad, kind = check_gaps(eng, tri, bounds)
    if how == "start":
        assert (bad, kind) == (at, 1)
    elif how == "class":
        assert (bad, kind) == ((at, 2) if tri[at, 0] < 0 else (-1, 0))
    else:
        assert (bad, kind) == (at, 2)
    if bad >= 0:
        assert g > at // 4 if at > 8 else g >= 0
        tri[at + 1:, 1] = 7                              # whatever follows the first bad region plays no part in the gaps
        assert check_gaps(eng, tri, bounds) == (g, bad, kind)


def test_every_region_a_run_of_its_own(eng):
    n = 2 * T + 5
    tri = np.stack([np.arange(n) % 2, np.full(n, 10), np.full(n, 20)], axis=1)
    assert check_gaps(eng, tri, [100, 100]) == (2 * n, -1, 0)                 # two gaps each; the ranks cross the spans and the tiles
    assert check_gaps(eng, tri, [100, 21]) == (2 * n - n // 2, -1, 0)         # one-base tails are not gaps
    assert check_pairs(eng, tri) == (2, 0, 0)                                 # ... and for the pair pass the classes go back at row 2


def test_capacity_zero_and_one_short(eng):
    tri = sorted_regions(9, 2 * T + 300, 4, 60 * T)
    bounds = [60 * T + 100] * 4
    need, _, _ = check_gaps(eng, tri, bounds)
    assert need > T
    for cap in (0, 1, need - 1, need, need + 7):
        assert check_gaps(eng, tri, bounds, capacity=cap)[0] == need
    # nothing is written behind the capacity
    o, s, e = np.full(need, 0xABCD, dtype=np.uint32), np.full(need, -7, dtype=np.int32), np.full(need, -7, dtype=np.int32)
    import ctypes
    info = gtx.GapsInfo()
    b = np.asarray(bounds, dtype=np.int64)
    eng._chk(eng.lib.gtx_gaps(eng.ctx, gtx._ptr(tri), len(tri), gtx._ptr(b), len(b), need - 1, gtx._ptr(o), gtx._ptr(s), gtx._ptr(e), ctypes.byref(info)))
    assert info.n_gaps == need and o[-1] == 0xABCD and s[-1] == -7 and e[-1] == -7 and o[-2] != 0xABCD


def test_coordinates_where_32_bits_wrap(eng):
    tri = [[0, -BIG, -BIG + 5], [0, BIG - 1, BIG]]
    dist, u, i, o = ar.adjacent_packed(tri, None, 0, 1)
    assert dist[1] == 2 * BIG and (u, i, o) == (-1, 0, 0)                     # a 32-bit difference would be negative
    check_pairs(eng, tri, None, 0, 1)
    check_pairs(eng, [[0, -BIG, BIG], [0, -BIG + 1, -BIG + 1]], None, 1, 0)   # -(2^32 - 7)
    check_pairs(eng, [[0, BIG, BIG + 2], [0, BIG, BIG + 2]])                  # STOP = 2^31 - 1
    # STOP + 1 in 64 bits: a region that ends at 2^31 - 1 has no gap behind it, and the next one none in front of it
    assert check_gaps(eng, [[0, 1, BIG + 2], [0, 5, BIG]], [BIG]) == (0, -1, 0)
    assert check_gaps(eng, [[0, 1, BIG - 2]], [BIG]) == (1, -1, 0)
    assert check_gaps(eng, [[0, 1, BIG - 1]], [BIG]) == (0, -1, 0)
    assert check_gaps(eng, [[0, -BIG, -BIG], [0, BIG, BIG]], [BIG]) == (1, -1, 0)        # [-BIG + 1, BIG - 1]


def test_zero_length_and_inverted_regions(eng):
    tri = sorted_regions(17, 2 * T + 77, 3, 3 * T, lmin=-4, lmax=12)          # ~2 regions per start
    minus = np.random.default_rng(5).integers(0, 2, size=len(tri)).astype(np.uint8)
    u, i, o = check_pairs(eng, tri, minus, 2, 3)
    assert u == -1 and i > 100 and o > 100
    assert check_gaps(eng, tri, [3 * T + 50] * 3)[0] > 100


@pytest.mark.parametrize("op1,op2", list(itertools.product(range(4), range(4))))
def test_all_point_pairs_with_random_strands(eng, op1, op2):
    tri = sorted_regions(31, T + 200, 6, 20 * T)
    minus = (tri[:, 0] & 1).astype(np.uint8)                                  # the strand is the class's low bit, as the tool packs it
    check_pairs(eng, tri, minus, op1, op2)
    mixed = np.random.default_rng(op1 * 4 + op2).integers(0, 2, size=len(tri)).astype(np.uint8)   # ... and strands that differ inside a class
    check_pairs(eng, tri, mixed, op1, op2)
    if op1 >= 2 or op2 >= 2:
        assert not np.array_equal(ar.adjacent_packed(tri, mixed, op1, op2)[0], ar.adjacent_packed(tri, None, op1, op2)[0])


@pytest.fixture(scope="module")
def big_sets():
    """200 000 regions over 24 classes, dense and sparse, and the restatement's answers, computed once"""
    sets = {}
    for name, span in (("dense", 40_000), ("sparse", 20_000_000)):
        tri = sorted_regions(len(name), 200_000, 24, span, 1, 60)
        minus = (tri[:, 0] & 1).astype(np.uint8)
        bounds = [span + 1000] * 24
        sets[name] = (tri, minus, bounds, ar.adjacent_packed(tri, minus, 2, 3), ar.gaps_packed(tri, bounds))
    return sets


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_200k_random_regions(eng, big_sets, name):
    tri, minus, bounds, (wd, wu, wi, wo), (go, gs, ge, gb, gk) = big_sets[name]
    dist, info = eng.adjacent(tri, minus, 2, 3, want_dist=True)
    assert info == {"first_unsorted": wu, "n_inclusions": wi, "n_overlaps": wo} and wu == -1
    np.testing.assert_array_equal(dist, wd)
    o, s, e, info = eng.gaps(tri, bounds)
    assert info == {"n_gaps": len(go), "first_bad": -1, "bad_kind": 0}
    np.testing.assert_array_equal(o, go)
    np.testing.assert_array_equal(s, gs)
    np.testing.assert_array_equal(e, ge)
    assert {"dense": wi + wo > 150_000 and len(go) < 20_000, "sparse": wi + wo < 5_000 and len(go) > 190_000}[name]


def test_more_bounds_than_fit_in_lds(eng):
    """above 4096 classes the bounds are read through L2: same answers"""
    n_classes = 5000
    tri = sorted_regions(41, T + 500, n_classes, 1000)
    bounds = np.full(n_classes, 1100, dtype=np.int64)
    bounds[tri[T, 0]] = -1
    g, bad, kind = check_gaps(eng, tri, bounds)
    assert kind == 2 and bad == int(np.flatnonzero(tri[:, 0] == tri[T, 0])[0]) and g > T // 2
    assert check_gaps(eng, tri, np.full(n_classes, 1100, dtype=np.int64))[1] == -1


def test_device_entries_on_torch_tensors_two_calls_and_one_sync(eng):
    """each call's info reaches its own struct, whether the next call or the sync is what waits for it"""
    import torch
    a = sorted_regions(21, 2 * T + 5, 3, 30 * T)
    b = sorted_regions(22, T + 9, 2, 4 * T).astype(np.int64)
    b[T // 2, 1] = b[T // 2 - 1, 1] - 1; b[T // 2, 0] = b[T // 2 - 1, 0]          # an unsorted region in the second input
    b = b.astype(np.int32)
    ma, mb = (a[:, 0] & 1).astype(np.uint8), (b[:, 0] & 1).astype(np.uint8)
    want_a, want_b = ar.adjacent_packed(a, ma, 2, 1), ar.adjacent_packed(b, mb, 0, 3)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dma, dmb = torch.from_numpy(ma).cuda(), torch.from_numpy(mb).cuda()
    oa, ob = torch.zeros(len(a), dtype=torch.int64, device="cuda"), torch.zeros(len(b), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ia = eng.adjacent_device(da.data_ptr(), len(a), dma.data_ptr(), 2, 1, oa.data_ptr())
    ib = eng.adjacent_device(db.data_ptr(), len(b), dmb.data_ptr(), 0, 3, ob.data_ptr())
    eng.sync()
    assert ia.as_dict() == {"first_unsorted": -1, "n_inclusions": want_a[2], "n_overlaps": want_a[3]}
    assert ib.as_dict() == {"first_unsorted": T // 2, "n_inclusions": want_b[2], "n_overlaps": want_b[3]}
    np.testing.assert_array_equal(oa.cpu().numpy(), want_a[0])
    np.testing.assert_array_equal(ob.cpu().numpy(), want_b[0])
    # the gaps of both, and a count-only pair pass between them
    bounds_a, bounds_b = [30 * T + 100] * 3, [4 * T + 100] * 2
    ga, gb = ar.gaps_packed(a, bounds_a), ar.gaps_packed(b, bounds_b)
    outs = []
    for n in (len(ga[0]), len(gb[0])):
        outs.append([torch.zeros(max(n, 1), dtype=torch.int32, device="cuda") for _ in range(3)])
    torch.cuda.synchronize()
    ja = eng.gaps_device(da.data_ptr(), len(a), bounds_a, len(ga[0]), *[t.data_ptr() for t in outs[0]])
    ic = eng.adjacent_device(da.data_ptr(), len(a))
    jb = eng.gaps_device(db.data_ptr(), len(b), bounds_b, len(gb[0]), *[t.data_ptr() for t in outs[1]])
    eng.sync()
    assert ja.as_dict() == {"n_gaps": len(ga[0]), "first_bad": -1, "bad_kind": 0} and len(ga[0]) > T
    assert jb.as_dict() == {"n_gaps": len(gb[0]), "first_bad": T // 2, "bad_kind": 1} and len(gb[0]) > 100
    assert ic.as_dict() == ia.as_dict()
    for want, out in ((ga, outs[0]), (gb, outs[1])):
        np.testing.assert_array_equal(out[0].cpu().numpy().view(np.uint32), want[0])
        np.testing.assert_array_equal(out[1].cpu().numpy(), want[1])
        np.testing.assert_array_equal(out[2].cpu().numpy(), want[2])
    del ia, ib, ic, ja, jb                                                       # dropped before the next sync: the binding keeps them alive
    eng.adjacent_device(da.data_ptr(), len(a))
    eng.sync()


def test_link_adjacent_and_gaps_infos_pending_under_one_sync(eng):
    """one device call of each family enqueued, then one sync: every info reaches its own struct and every output is the packed loop's"""
    import torch
    import link_restate
    a = sorted_regions(21, 2 * T + 5, 3, 30 * T)
    ma = (a[:, 0] & 1).astype(np.uint8)
    bounds = [30 * T + 100] * 3
    want_l, want_a, want_g = link_restate.link_packed(a, 0), ar.adjacent_packed(a, ma, 2, 1), ar.gaps_packed(a, bounds)
    n, ng = len(a), len(want_g[0])
    da, dma = torch.from_numpy(a).cuda(), torch.from_numpy(ma).cuda()
    ol = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    od = torch.zeros(n, dtype=torch.int64, device="cuda")
    og = [torch.zeros(max(ng, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    il = eng.link_device(da.data_ptr(), n, ol[0].data_ptr(), ol[1].data_ptr(), ol[2].data_ptr(), None, None, 0, 0)
    ia = eng.adjacent_device(da.data_ptr(), n, dma.data_ptr(), 2, 1, od.data_ptr())
    ig = eng.gaps_device(da.data_ptr(), n, bounds, ng, *[t.data_ptr() for t in og])
    eng.sync()
    groups = len(want_l[0])
    assert il.as_dict() == {"n_groups": groups, "first_unsorted": want_l[4]} and groups > 1 and want_l[4] == -1
    assert ia.as_dict() == {"first_unsorted": want_a[1], "n_inclusions": want_a[2], "n_overlaps": want_a[3]}
    assert ig.as_dict() == {"n_gaps": ng, "first_bad": want_g[3], "bad_kind": want_g[4]} and ng > T
    np.testing.assert_array_equal(ol[0].cpu().numpy().view(np.uint32)[:groups], want_l[0])
    np.testing.assert_array_equal(ol[1].cpu().numpy().view(np.uint32)[:groups], want_l[1])
    np.testing.assert_array_equal(ol[2].cpu().numpy()[:groups], want_l[2])
    np.testing.assert_array_equal(od.cpu().numpy(), want_a[0])
    np.testing.assert_array_equal(og[0].cpu().numpy().view(np.uint32), want_g[0])
    np.testing.assert_array_equal(og[1].cpu().numpy(), want_g[1])
    np.testing.assert_array_equal(og[2].cpu().numpy(), want_g[2])
    del il, ia, ig                                                               # dropped before the next sync: the binding keeps them alive
    eng.link_device(da.data_ptr(), n, ol[0].data_ptr(), ol[1].data_ptr(), ol[2].data_ptr(), None, None, 0, 0)
    eng.adjacent_device(da.data_ptr(), n)
    eng.sync()


def test_bad_arguments(eng):
    tri = sorted_regions(1, 10, 1, 100)
    for op1, op2 in ((4, 0), (0, 4), (-1, 0), (0, -1)):
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            eng.adjacent(tri, None, op1, op2)
    with pytest.raises(gtx.GtxError, match="gtx error -4"):
        eng.gaps(tri, [2**31 - 2])                                   # a bound above 2^31 - 3
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        eng.gaps(tri, [100], capacity=-1)
    import ctypes
    info = gtx.AdjacentInfo()
    assert eng.lib.gtx_adjacent(eng.ctx, gtx._ptr(tri), None, 2**32, 0, 0, None, ctypes.byref(info)) == -1      # n < 2^32
    assert eng.lib.gtx_adjacent(eng.ctx, gtx._ptr(tri), None, 10, 0, 0, None, None) == -1
    ginfo = gtx.GapsInfo()
    assert eng.lib.gtx_gaps(eng.ctx, gtx._ptr(tri), 2**32, None, 0, 0, None, None, None, ctypes.byref(ginfo)) == -1
    assert check_gaps(eng, tri, [2**31 - 3])[1] == -1                # the largest bound; the context is still good
    assert check_gaps(eng, tri, []) == (0, 0, 2)                     # no bounds at all: the first head has none
    check_pairs(eng, tri)


@pytest.fixture(scope="module")
def many_spans():
    """1025 spans of 512 regions and one more region, over 24 classes at a density where the spans differ in their number of gaps"""
    n = 1025 * 512 + 1
    return sorted_regions(78, n, 24, 2 * n, 1, 60).astype(np.int64)


@pytest.mark.parametrize("bad", [False, True], ids=["clean", "bad-in-the-last-tile"])
def test_more_spans_than_threads_in_the_gaps_prefix(eng, many_spans, bad):
    """The one-block exclusive sum of the spans' gap counts (block_exclusive_sum, csrc/gtx_compact.h) with two spans to a thread and
    the upper half of its threads without one.  With a region of span 1024 that starts before its predecessor, the gaps that count
    are read behind that sum at a base that is not zero, and those of its span below it are added."""
    tri = many_spans.copy()
    at = 1024 * 512 + 300
    if bad:
        tri[at, 0] = tri[at - 1, 0]
        tri[at, 1] = tri[at - 1, 1] - 1
    n_gaps, first_bad, kind = check_gaps(eng, tri, [BIG] * 24)
    assert (first_bad, kind) == ((at, 1) if bad else (-1, 0))
    assert len(tri) // 8 < n_gaps < len(tri)
    per_span = np.bincount(eng.gaps(tri, [BIG] * 24)[0] // 512, minlength=1026)
    assert len(set(per_span[:1024].tolist())) > 8                                # the spans' counts vary
