"""The window filter on the device (gtx_window_refs / gtx_window_filter / gtx_window_filter_device, csrc/gtx_filter.hip) through the C
ABI, on synthetic uint64 vectors: the expected answers are the brute-force restatement's (tests/window_filter_restate.py: every
(window, region) pair), the shapes are placed by GTX_FILTER_TILE."""
import os
import re

import numpy as np
import pytest
import torch

import gtx
import window_filter_restate as wf

pytestmark = pytest.mark.gpu

T = gtx.FILTER_TILE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = gtx.Engine(0)
    yield e
    e.close()


def on_device(v):
    """a uint64 vector in HBM (as its int64 bits); at least one element so that the address is real"""
    a = np.ascontiguousarray(v, dtype=np.uint64)
    return torch.from_numpy(np.concatenate([a, np.zeros(2, dtype=np.uint64)]).view(np.int64)).cuda()


def class_of(n_win, step, size, extra=0):
    """a class length with exactly n_win windows (n_win = 0: shorter than one window)"""
    return size - 1 if n_win == 0 else (n_win - 1) * step + size + extra


def tiled_layout(step, size):
    """about 3 T + 5 windows over five classes, their offsets not in class order: vector order is class 3, 0, 4 (none), 2, then a gap
    of 7 ordinals, then 1.  Class 0 ends in the middle of tile 1, class 2 in the middle of tile 2."""
    counts = [T, T // 2 + 3, T - 9, T // 2 + 4, 0]
    order = [3, 0, 4, 2, 1]
    off, at = [0] * 5, 0
    for c in order:
        if c == 1:
            at += 7
        off[c] = at
        at += counts[c]
    class_len = [class_of(n, step, size, extra=(c * 3) % step) for c, n in enumerate(counts)]
    assert [wf.n_windows(ln, step, size) for ln in class_len] == counts and at == 3 * T + 5
    return class_len, np.asarray(off, dtype=np.int64), at


def check(eng, values, class_len, off, step, size, refs, min_value=0):
    want_o, want_v = wf.keep_brute(values, class_len, off, step, size, refs, min_value)
    eng.window_refs(refs, class_len, off, step, size)
    d = on_device(values)
    o, v, kept = eng.window_filter(d.data_ptr(), min_value, n_windows=len(values))
    torch.cuda.synchronize()
    assert kept == len(want_o)
    np.testing.assert_array_equal(o, want_o); np.testing.assert_array_equal(v, want_v)
    return want_o


def test_the_tile_is_what_the_header_names():
    src = open(os.path.join(ROOT, "include", "gtx.h")).read()
    assert int(re.search(r"#define\s+GTX_FILTER_TILE\s+(\d+)", src).group(1)) == T and T % 128 == 0


@pytest.mark.parametrize("step,size", [(25, 25), (25, 500), (7, 21)], ids=["W=D", "W=20D", "W=3D"])
@pytest.mark.parametrize("min_value", [0, 1, 3])
def test_classes_across_tiles_gaps_and_a_class_without_a_window(eng, step, size, min_value):
    class_len, off, n = tiled_layout(step, size)
    rng = np.random.default_rng(step + size + min_value)
    values = rng.integers(0, 5, size=n).astype(np.uint64)
    m = 250
    cls = rng.integers(0, 5, size=m)
    s = rng.integers(-size, max(class_len) + size, size=m)
    refs = np.stack([cls, s, s + rng.integers(0, 4 * step, size=m)], axis=1)
    kept = check(eng, values, class_len, off, step, size, refs, min_value)
    assert 0 < len(kept) < n
    gap = np.arange(off[1] - 7, off[1])
    assert not np.isin(gap, kept).any()                                         # ordinals that belong to no class


@pytest.mark.parametrize("step,size", [(25, 25), (25, 500)], ids=["W=D", "W=20D"])
def test_regions_that_touch_a_window_edge(eng, step, size):
    class_len, off, n = tiled_layout(step, size)
    values = np.ones(n, dtype=np.uint64)
    comb = size // step
    c = 0                                                                        # class 0 lies at ordinals T // 2 + 4 .. : its window k = T // 2 - 5 is ordinal T - 1
    k = T - 1 - int(off[c])
    assert 0 < k - comb and k + comb + 1 < wf.n_windows(class_len[c], step, size)
    def kept_in_class(refs):
        return set((check(eng, values, class_len, off, step, size, refs) - off[c]).tolist())
    # s = D k + W: the last position of window k
    got = kept_in_class([[c, step * k + size, step * k + size]])
    assert k in got and k - 1 not in got and got == set(range(k, k + comb))
    # s = D k + W + 1: window k is not reached any more
    got = kept_in_class([[c, step * k + size + 1, step * k + size + 1]])
    assert k not in got and got == set(range(k + 1, k + 1 + comb))
    # e = D k + 1: the first position of window k
    got = kept_in_class([[c, step * k + 1, step * k + 1]])
    assert k in got and k + 1 not in got and got == set(range(k - comb + 1, k + 1))
    # e = D k: window k is not reached
    got = kept_in_class([[c, step * k, step * k]])
    assert k not in got and k - 1 in got and got == set(range(k - comb, k))
    # the last lane of tile 0 and the first lane of tile 1, and nothing else of either tile (W = D), from one region
    if comb == 1:
        at = check(eng, values, class_len, off, step, size, [[c, step * k + size, step * (k + 1) + 1]])
        assert at.tolist() == [T - 1, T]


def test_a_long_region_in_front_of_many_short_ones(eng):
    step, size = 10, 10
    class_len, off, n = tiled_layout(step, size)
    values = np.full(n, 2, dtype=np.uint64)
    c = 3                                                                        # class 3 is ordinals 0 .. T - 1; class 0 follows
    long_one = [0, 55, step * (T - 40)]                                           # class 0: from tile 0 into tile 1
    wide = [2, 31, step * (T - 20)]                                              # class 2 (T - 9 windows from ordinal T + T // 2 + 7): spans tiles 1 and 2
    rng = np.random.default_rng(9)
    short = [[2, 40 + 3 * j, 40 + 3 * j + int(rng.integers(0, 6))] for j in range(300)]   # behind `wide` in start order, all ending before 1000
    refs = [long_one, wide] + short + [[c, 5, 6]]
    order = rng.permutation(len(refs))
    kept = check(eng, values, class_len, off, step, size, [refs[j] for j in order])
    far = int(off[2]) + (step * (T - 20) - 1) // step                            # the window that holds wide's last position: beyond every short region
    assert far in kept and far + 1 not in kept and far // T == 2 and (int(off[2]) + 3) // T == 1
    assert int(off[2]) + 500 in kept                                             # inside `wide`, a tile away from any short region
    # a region over more than two tiles in one class
    class_len2 = [class_of(3 * T + 5, step, size)]
    refs2 = [[0, 25, step * (2 * T + 700)]] + [[0, 30 + 2 * j, 33 + 2 * j] for j in range(200)]
    kept = check(eng, np.full(3 * T + 5, 2, dtype=np.uint64), class_len2, np.zeros(1, dtype=np.int64), step, size, refs2)
    assert kept.tolist() == list(range(2, 2 * T + 700))


def test_clamped_dropped_duplicate_and_other_strand_regions(eng):
    step, size = 5, 10
    class_len, off, n = tiled_layout(step, size)
    values = np.full(n, 1, dtype=np.uint64)
    assert check(eng, values, class_len, off, step, size, [[0, -40, 3]]).tolist() == [int(off[0])]           # s <= 0 counts as 1
    assert check(eng, values, class_len, off, step, size, [[0, -40, 0], [0, -9, -2], [2, 50, 49], [2, 2**31 - 1, 5]]).tolist() == []   # e <= 0, s > e
    one = check(eng, values, class_len, off, step, size, [[2, 100, 130]])
    dup = check(eng, values, class_len, off, step, size, [[2, 100, 130]] * 7 + [[2, 50, 49]] * 3 + [[2, 100, 130]])
    assert one.tolist() == dup.tolist() and len(one) == 8
    # classes 0 and 1 as the two strands of one chromosome: a region on '-' only keeps no '+' window
    only_minus = check(eng, values, class_len, off, step, size, [[1, 20, 400]])
    assert len(only_minus) > 0 and (only_minus >= off[1]).all()
    assert check(eng, values, class_len, off, step, size, [[4, 1, 100]]).tolist() == []                          # the class without a window


def test_a_tile_no_region_reaches_emits_nothing(eng):
    step, size = 25, 500
    n = 4 * T
    class_len = [class_of(n, step, size)]
    off = np.zeros(1, dtype=np.int64)
    values = np.full(n, 50, dtype=np.uint64)                                      # every window would pass the value test
    first_of_tile_2 = step * (2 * T) + 1
    refs = [[0, 10, 30], [0, first_of_tile_2 - size - 1 - step, first_of_tile_2 - size - step], [0, step * (3 * T) + size, step * (3 * T) + size + 3]]
    kept = check(eng, values, class_len, off, step, size, refs, 10)
    assert len(kept) > 0 and not ((kept >= 2 * T) & (kept < 3 * T)).any() and (kept // T == 3).any() and (kept // T == 1).any()


def test_no_regions_and_no_windows(eng):
    class_len, off, n = tiled_layout(25, 50)
    values = np.full(n, 9, dtype=np.uint64)
    assert check(eng, values, class_len, off, 25, 50, np.zeros((0, 3), dtype=np.int32)).tolist() == []
    eng.window_refs([[0, 1, 10]], [10], [0], 25, 50)                            # a geometry without a window
    o, v, kept = eng.window_filter(on_device(np.zeros(0, dtype=np.uint64)).data_ptr(), 0, n_windows=0)
    assert kept == 0 and len(o) == 0


def test_min_values_and_values_beyond_32_bits(eng):
    step, size = 25, 25
    class_len, off, n = tiled_layout(step, size)
    rng = np.random.default_rng(3)
    values = rng.integers(0, 4, size=n).astype(np.uint64)
    values[[5, T - 1, T, 2 * T + 3]] = [2**32, 2**32 + 1, 2**40, 2**63 + 2]      # low words 0, 1, 0, 2
    refs = [[c, 1, 2**31 - 2] for c in range(5)]                                  # every window of every class
    assert len(check(eng, values, class_len, off, step, size, refs, 0)) == n - 7
    assert 0 < len(check(eng, values, class_len, off, step, size, refs, 1)) < n - 7
    assert check(eng, values, class_len, off, step, size, refs, 4).tolist() == [5, T - 1, T, 2 * T + 3]
    assert check(eng, values, class_len, off, step, size, refs, 2**32 + 1).tolist() == [T - 1, T, 2 * T + 3]
    assert check(eng, values, class_len, off, step, size, refs, 2**63 + 2).tolist() == [2 * T + 3]
    assert check(eng, values, class_len, off, step, size, refs, 2**63 + 3).tolist() == []   # above every value


def test_capacity_one_short_none_then_enough(eng):
    step, size = 25, 100
    class_len, off, n = tiled_layout(step, size)
    rng = np.random.default_rng(8)
    values = rng.integers(0, 5, size=n).astype(np.uint64)
    refs = np.stack([rng.integers(0, 4, size=160), rng.integers(1, 30000, size=160)], axis=1)
    refs = np.concatenate([refs, refs[:, 1:] + rng.integers(0, 900, size=(160, 1))], axis=1)
    want_o, want_v = wf.keep_brute(values, class_len, off, step, size, refs, 2)
    assert len(want_o) > T // 2 and want_o[0] < T and want_o[-1] > 2 * T
    eng.window_refs(refs, class_len, off, step, size)
    d = on_device(values)
    cap = len(want_o) - 1
    o, v, kept = eng.window_filter(d.data_ptr(), 2, n_windows=n, capacity=cap)
    assert kept == len(want_o) and len(o) == cap
    np.testing.assert_array_equal(o, want_o[:cap]); np.testing.assert_array_equal(v, want_v[:cap])
    # the device form: nothing is written behind the capacity
    for cap in (len(want_o) - 1, 0):
        d_o = torch.full((len(want_o) + 64,), -7, dtype=torch.int64, device="cuda")
        d_v = torch.full((len(want_o) + 64,), -7, dtype=torch.int64, device="cuda")
        kept = eng.window_filter(d.data_ptr(), 2, n_windows=n, capacity=cap, device_out=(d_o.data_ptr(), d_v.data_ptr()))
        torch.cuda.synchronize()
        assert kept == len(want_o)
        ho, hv = d_o.cpu().numpy(), d_v.cpu().numpy()
        np.testing.assert_array_equal(ho[:cap], want_o[:cap]); np.testing.assert_array_equal(hv[:cap].view(np.uint64), want_v[:cap])
        assert (ho[cap:] == -7).all() and (hv[cap:] == -7).all()
    o, v, kept2 = eng.window_filter(d.data_ptr(), 2, n_windows=n, capacity=kept)  # a second call with the reported count is the full answer
    assert kept2 == kept
    np.testing.assert_array_equal(o, want_o); np.testing.assert_array_equal(v, want_v)
    assert eng.window_filter(d.data_ptr(), 2, n_windows=n, capacity=0)[2] == len(want_o)


def test_error_codes():
    e = gtx.Engine(0)
    try:
        d = on_device(np.zeros(64, dtype=np.uint64))
        with pytest.raises(gtx.GtxError, match="gtx error -3"):
            e.window_filter(d.data_ptr(), 0, n_windows=16)                       # before gtx_window_refs
        with pytest.raises(gtx.GtxError, match="gtx error -3"):
            e.window_filter(d.data_ptr(), 0, n_windows=16, capacity=4, device_out=(d.data_ptr(), d.data_ptr()))
        class_len, off = [class_of(16, 5, 10), class_of(8, 5, 10)], [0, 16]
        for bad in ([[2, 1, 5]], [[0, 1, 5], [-1, 1, 5]], [[0, 9, 3], [7, 9, 3]]):  # (a region that takes no part is checked too)
            with pytest.raises(gtx.GtxError, match="gtx error -4"):
                e.window_refs(bad, class_len, off, 5, 10)
        with pytest.raises(gtx.GtxError, match="gtx error -3"):
            e.window_filter(d.data_ptr(), 0, n_windows=24)                       # a refused set is no set
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            e.window_refs([[0, 1, 5]], class_len, [0, 15], 5, 10)                # two classes share an ordinal
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            e.window_refs([[0, 1, 5]], class_len, off, 5, 12)                    # size no multiple of step
        e.window_refs([[0, 1, 5]], class_len, off, 5, 10)
        assert e.window_filter(d.data_ptr(), 0, n_windows=24)[0].tolist() == [0]
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            e.window_filter(d.data_ptr() + 8, 0, n_windows=24)                   # not 16-byte aligned
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            e.window_filter(d.data_ptr(), 0, n_windows=24, capacity=4, device_out=(None, d.data_ptr()))   # null output
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            e.window_filter(d.data_ptr(), 0, n_windows=24, capacity=4, device_out=(d.data_ptr(), None))
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            e.window_filter(d.data_ptr(), 0, n_windows=23)                       # class 1 reaches beyond the vector
        assert e.window_filter(d.data_ptr(), 0, n_windows=24, capacity=0, device_out=(None, None)) == 1    # no room asked for: no buffer needed
    finally:
        e.close()


@pytest.mark.parametrize("seed", range(20))
def test_seeded_shapes(eng, seed):
    rng = np.random.default_rng(100 + seed)
    class_len, step, size, refs = wf.random_case(rng, 4 * T, 300)
    n_classes = len(class_len)
    counts = [wf.n_windows(ln, step, size) for ln in class_len]
    order = rng.permutation(n_classes)                                           # offsets in no class order, with gaps now and then
    off, at = np.zeros(n_classes, dtype=np.int64), 0
    for c in order:
        at += int(rng.integers(0, 3)) * int(rng.integers(0, 40))
        off[c] = at
        at += counts[c]
    assert at <= 4 * T + 6 * 80
    values = rng.integers(0, 4, size=at).astype(np.uint64)
    for min_value in (0, int(rng.integers(1, 4))):
        check(eng, values, class_len, off, step, size, refs, min_value)
