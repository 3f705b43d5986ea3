"""The peak candidate selection on the device (gtx_peak_select / gtx_peak_select_device, csrc/gtx_peaks.hip) through the C ABI, on
synthetic uint64 vectors: the expected answers are the numpy restatement's (tests/peaks_select_restate.py, pinned by hand-derived
vectors in tests/test_peaks_select_restate_cpu.py), the shapes are placed by GTX_PEAK_TILE."""
import json
import os
import re

import numpy as np
import pytest
import torch

import gtx
import peaks_select_restate as ps

pytestmark = pytest.mark.gpu

T = gtx.PEAK_TILE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, T - 1, T, T + 1, 3 * T + 5]


@pytest.fixture(scope="module")
def eng():
    e = gtx.Engine(0)
    yield e
    e.close()


def on_device(v):
    """a uint64 vector in HBM (as its int64 bits); at least one element so that the address is real"""
    a = np.ascontiguousarray(v, dtype=np.uint64)
    return torch.from_numpy(np.concatenate([a, np.zeros(2, dtype=np.uint64)]).view(np.int64)).cuda()


def check(eng, S, C, U, win_size, min_reads, norm=False, p_ratio=1.0):
    want_o, want_r = ps.select(S, C, U, win_size, min_reads, norm, p_ratio)
    dS, dC, dU = on_device(S), on_device(C), None if U is None else on_device(U)
    o, r, kept = eng.peak_select(dS.data_ptr(), dC.data_ptr(), win_size, min_reads, uniq=None if dU is None else dU.data_ptr(), norm=norm, p_ratio=p_ratio,
                                 n_windows=len(S))
    torch.cuda.synchronize()
    assert kept == len(want_o)
    np.testing.assert_array_equal(o, want_o); np.testing.assert_array_equal(r, want_r)
    return want_o


def vectors(n, seed, hi=30):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, hi, size=n).astype(np.uint64), rng.integers(0, hi, size=n).astype(np.uint64), rng.integers(0, hi, size=n).astype(np.uint64))


def test_the_tile_is_what_the_header_names():
    src = open(os.path.join(ROOT, "include", "gtx.h")).read()
    assert int(re.search(r"#define\s+GTX_PEAK_TILE\s+(\d+)", src).group(1)) == T and T % 128 == 0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("with_u", [False, True], ids=["W", "U"])
def test_sizes_around_the_tile(eng, n, with_u):
    S, C, U = vectors(n, 7 + n)
    kept = check(eng, S, C, U if with_u else None, 20, 10)
    assert n < 2 or 0 < len(kept) < n
    check(eng, S, C, U if with_u else None, 20, 10, norm=True, p_ratio=0.37)
    check(eng, S, C, U if with_u else None, 20, 10, norm=True, p_ratio=2.6)


@pytest.mark.parametrize("n", SIZES[1:])
def test_nothing_and_everything_kept(eng, n):
    S, C, U = vectors(n, 11 + n)
    assert len(check(eng, S, C, None, 20, 21)) == 0                              # above the clamp: nothing
    assert len(check(eng, S, C, U, 20, 1000)) == 0
    assert len(check(eng, S, C, None, 20, 0)) == n                               # min_reads = 0: everything, zeros included
    assert len(check(eng, S, C, U, 20, 0)) == n
    assert len(check(eng, S, C, U, 20, -5)) == n
    assert len(check(eng, S, C, None, 20, -5, norm=True, p_ratio=2.6)) == n


def test_kept_windows_in_one_tile_only_and_in_the_last_window(eng):
    n = 3 * T + 5
    C = np.full(n, 3, dtype=np.uint64)
    for where in (np.arange(0, T), np.arange(3 * T, n), np.array([n - 1]), np.array([0]), np.array([T + 17])):
        S = np.zeros(n, dtype=np.uint64)
        S[where] = 15
        for U in (None, np.full(n, 40, dtype=np.uint64)):
            assert check(eng, S, C, U, 20, 10).tolist() == where.tolist()


@pytest.mark.parametrize("with_u", [False, True], ids=["W", "U"])
def test_a_kept_window_on_each_side_of_every_tile_seam(eng, with_u):
    n = 3 * T + 5
    seams = np.array([T - 1, T, 2 * T - 1, 2 * T, 3 * T - 1, 3 * T])
    S = np.zeros(n, dtype=np.uint64)
    S[seams] = 12 + np.arange(6, dtype=np.uint64)
    C = np.arange(n, dtype=np.uint64) % 7
    U = np.full(n, 16, dtype=np.uint64) if with_u else None
    assert check(eng, S, C, U, 20, 10).tolist() == seams.tolist()
    # ... and the 128-window rows inside a tile, where the rank passes from the ballots to the running count
    rows = np.array([127, 128, 255, 256, T + 127, T + 128])
    S[:] = 0
    S[rows] = 11
    assert check(eng, S, C, U, 20, 10).tolist() == rows.tolist()


@pytest.mark.parametrize("p_ratio", [0.37, 2.6, 0.5, 1.0, 1.5])
def test_norm_rounds_the_count_to_float_first(eng, p_ratio):
    n = T + 1
    rng = np.random.default_rng(5)
    S = rng.integers(0, 50, size=n).astype(np.uint64)
    C = rng.integers(0, 50, size=n).astype(np.uint64)
    big = np.array([2**24 + 1, 2**24 + 3, 2**25 + 2, 2**31 + 129, 2**40 + 2**16 + 1], dtype=np.uint64)
    S[[3, T - 1, T]] = big[[0, 1, 3]]
    C[[3, 5, T]] = big[[0, 2, 4]]
    for min_reads in (10, 2**24):
        check(eng, S, C, None, 2**41, min_reads, norm=True, p_ratio=p_ratio)
    U = np.full(n, 2**41, dtype=np.uint64)
    U[3] = 2**24 + 1                                                             # the clamp itself is the value that rounds
    check(eng, S + np.uint64(5), C + np.uint64(5), U, 500, 10, norm=True, p_ratio=p_ratio)


def test_the_hand_derived_vectors(eng):
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "peaks_select_manifest.json")))["cases"]
    for c in cases:
        S, C = np.array(c["S"], dtype=np.uint64), np.array(c["C"], dtype=np.uint64)
        U = None if c["U"] is None else np.array(c["U"], dtype=np.uint64)
        at = check(eng, S, C, U, c["win_size"], c["min_reads"], bool(c["norm"]), c["p_ratio"])
        assert at.tolist() == c["ordinals"]


def test_values_beyond_32_bits_and_signed_reading(eng):
    n = T + 1
    S, C, U = vectors(n, 3, hi=4)
    S[[5, T - 1, T]] = np.array([2**32, 2**32 + 1, 2**63 + 2], dtype=np.uint64)                            # low words 0, 1, 2; the last one is negative as a long
    C[[5, 6]] = np.array([2**35, 2**64 - 1], dtype=np.uint64)
    assert check(eng, S, C, None, 2**33, 4).tolist() == [5, T - 1]
    assert check(eng, S, C, None, 2**33, 2**32 + 1).tolist() == [T - 1]
    assert len(check(eng, S, C, None, 2**33, -(2**63))) == n
    U[:] = 2**34
    assert check(eng, S, C, U, 7, 2**32).tolist() == [5, T - 1]


def test_capacity_none_one_short_then_enough(eng):
    n = 3 * T + 5
    S, C, U = vectors(n, 8)
    want_o, want_r = ps.select(S, C, U, 20, 9, True, 0.37)
    assert len(want_o) > T // 2 and want_o[0] < T and want_o[-1] > 3 * T
    dS, dC, dU = on_device(S), on_device(C), on_device(U)
    args = dict(uniq=dU.data_ptr(), norm=True, p_ratio=0.37, n_windows=n)
    cap = len(want_o) - 1
    o, r, kept = eng.peak_select(dS.data_ptr(), dC.data_ptr(), 20, 9, capacity=cap, **args)
    assert kept == len(want_o) and len(o) == cap
    np.testing.assert_array_equal(o, want_o[:cap]); np.testing.assert_array_equal(r, want_r[:cap])
    # the device entry on raw addresses: the exact prefix, and nothing behind the capacity
    for cap in (len(want_o), len(want_o) - 1, 0):
        d_o = torch.full((len(want_o) + 64,), -7, dtype=torch.int64, device="cuda")
        d_r = torch.full((3 * (len(want_o) + 64),), -7, dtype=torch.int64, device="cuda")
        kept = eng.peak_select_device(dS.data_ptr(), dC.data_ptr(), 20, 9, cap, d_o.data_ptr(), d_r.data_ptr(), **args)
        torch.cuda.synchronize()
        assert kept == len(want_o)
        ho, hr = d_o.cpu().numpy(), d_r.cpu().numpy()
        np.testing.assert_array_equal(ho[:cap], want_o[:cap]); np.testing.assert_array_equal(hr[:3 * cap].reshape(-1, 3), want_r[:cap])
        assert (ho[cap:] == -7).all() and (hr[3 * cap:] == -7).all()
    o, r, kept2 = eng.peak_select(dS.data_ptr(), dC.data_ptr(), 20, 9, capacity=kept, **args)   # a second call with the reported count is the full answer
    assert kept2 == kept
    np.testing.assert_array_equal(o, want_o); np.testing.assert_array_equal(r, want_r)
    assert eng.peak_select(dS.data_ptr(), dC.data_ptr(), 20, 9, capacity=0, **args)[2] == len(want_o)


def test_kept_slots_as_inputs(eng):
    class_len, step, size = [40000, 2500], 25, 500
    rng = np.random.default_rng(2)
    def reads(n):
        c = rng.integers(0, 2, size=n)
        s = (rng.random(n) ** 2 * (np.asarray(class_len)[c] - 40)).astype(np.int64) + 1
        return np.stack([c, s, s + 30], axis=1).astype(np.int32)
    rs, rc = reads(3000), reads(2000)
    eng.scan_keep(0, rs, class_len, step, size, flags=gtx.READS_UNSORTED)
    eng.scan_keep(1, rc, class_len, step, size, flags=gtx.READS_UNSORTED)
    S, _ = eng.scan(rs, class_len, step, size)
    C, _ = eng.scan(rc, class_len, step, size)
    want_o, want_r = ps.select(S, C, None, size, 30)
    o, r, kept = eng.peak_select(0, 1, size, 30)
    assert kept == len(want_o) and 0 < kept < len(S)
    np.testing.assert_array_equal(o, want_o); np.testing.assert_array_equal(r, want_r)
    with pytest.raises(ValueError, match="n_windows"):
        eng.peak_select(eng.scan_kept(0)[0], 1, size, 30)                       # a raw address says nothing about its length
    eng.scan_drop()


@pytest.mark.parametrize("step,size,weighted", [(25, 500, False), (100, 100, True)], ids=["w500d25", "w100d100-weighted"])
def test_a_kept_slot_read_back_is_the_scan(eng, step, size, weighted):
    """gtx_scan_kept_read against gtx_scan on the same reads: classes of several lengths, one without a window, one slot beside another"""
    class_len = [40000, 2500, size - 1, 3 * gtx.PEAK_TILE * step + size]
    rng = np.random.default_rng(step)
    c = rng.integers(0, 4, size=5000)
    s = (rng.random(5000) * np.maximum(np.asarray(class_len)[c] - 40, 1)).astype(np.int64) + 1
    reads = np.stack([c, s, s + 30], axis=1).astype(np.int32)
    w = rng.integers(1, 5, size=5000).astype(np.int32) if weighted else None
    want, _ = eng.scan(reads, class_len, step, size, weights=w)
    assert want.sum() > 0
    eng.scan_keep(3, reads, class_len, step, size, weights=w, flags=gtx.READS_UNSORTED)
    eng.scan_keep(4, reads[:100], class_len, step, size, weights=None if w is None else w[:100], flags=gtx.READS_UNSORTED)
    got = eng.scan_kept_read(3)
    assert got.dtype == np.uint64
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(eng.scan_kept_read(3), want)                  # the slot stays as it is
    np.testing.assert_array_equal(eng.scan_kept_read(4), eng.scan(reads[:100], class_len, step, size, weights=None if w is None else w[:100])[0])
    eng.scan_drop(3)
    with pytest.raises(gtx.GtxError, match="gtx error -3"):
        eng.scan_kept(3)                                                        # an empty slot
    with pytest.raises(gtx.GtxError, match="gtx error -3"):
        eng.scan_kept_read(3)
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        eng._chk(eng.lib.gtx_scan_kept_read(eng.ctx, gtx.SCAN_KEEP_SLOTS, None))
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        eng._chk(eng.lib.gtx_scan_kept_read(eng.ctx, 4, None))                  # a slot that holds windows, no buffer
    eng.scan_drop()


def test_error_codes():
    e = gtx.Engine(0)
    try:
        d = on_device(np.arange(64, dtype=np.uint64))
        p = d.data_ptr()
        out = torch.zeros(256, dtype=torch.int64, device="cuda").data_ptr()
        def dev(signal=p, control=p, uniq=None, n=16, win=20, norm=False, ratio=1.0, cap=4, o=out, r=out):
            return e.peak_select_device(signal, control, win, 5, cap, o, r, uniq=uniq, norm=norm, p_ratio=ratio, n_windows=n)
        assert dev() == 11
        bad = [dict(signal=p + 8), dict(control=p + 8), dict(uniq=p + 8), dict(signal=None), dict(control=None), dict(o=None), dict(r=None), dict(win=0),
               dict(win=-3), dict(n=-1), dict(cap=-1), dict(norm=True, ratio=0.0), dict(norm=True, ratio=-1.5), dict(norm=True, ratio=float("inf")),
               dict(norm=True, ratio=float("nan")), dict(signal=None, n=0)]
        for kw in bad:
            with pytest.raises(gtx.GtxError, match="gtx error -1"):
                dev(**kw)
        assert dev(norm=False, ratio=float("nan")) == 11                         # the ratio is not looked at without norm
        assert dev(cap=0, o=None, r=None) == 11                                  # no room asked for: no buffer needed
        assert dev(n=0) == 0
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            e.peak_select(p + 8, p, 20, 5, n_windows=16)
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            e.peak_select(p, p, 20, 5, norm=True, p_ratio=0.0, n_windows=16)
        o, r, kept = e.peak_select(p, p, 20, 5, n_windows=0)
        assert kept == 0 and len(o) == 0
    finally:
        e.close()


@pytest.mark.parametrize("seed", range(12))
def test_seeded_shapes(eng, seed):
    rng = np.random.default_rng(300 + seed)
    n = int(rng.integers(1, 4 * T))
    hi = int(rng.choice([3, 40, 2**26]))
    S, C, U = (rng.integers(0, hi, size=n).astype(np.uint64) for _ in range(3))
    win = int(rng.choice([20, 500, 2**30]))
    for min_reads in (0, int(rng.integers(1, 12)), hi // 2):
        for norm, ratio in ((False, 1.0), (True, float(rng.uniform(0.05, 0.99))), (True, float(rng.uniform(1.0, 9.0)))):
            check(eng, S, C, U if seed % 2 else None, win, min_reads, norm, ratio)
