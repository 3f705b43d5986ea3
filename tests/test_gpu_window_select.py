"""The window selection on the device (gtx_window_select / gtx_window_select_device, csrc/gtx_select.hip) through the C ABI, on
synthetic uint64 vectors against a numpy statement of the rule: with k_f = min(v_f, W) and c_f = min(ctl_f, W) a window is kept when
k_f >= kcrit_f[c_f] for any tested f; the kept windows' ordinals and clamped rows come out in window order.  Shapes are placed by
gtx_window_select_limits."""
import numpy as np
import pytest
import torch

import gtx

pytestmark = pytest.mark.gpu

TILE, LDS_MAX_W = gtx.window_select_limits()


@pytest.fixture(scope="module")
def eng():
    e = gtx.Engine(0)
    yield e
    e.close()


def rule(tested, controls, tables, W):
    k = [np.minimum(v, np.uint64(W)).astype(np.int64) for v in tested]
    c = [np.minimum(v, np.uint64(W)).astype(np.int64) for v in controls]
    keep = np.zeros(len(tested[0]), dtype=bool)
    for f in range(len(tested)):
        keep |= k[f] >= (tables[f][c[f]] if controls else tables[f][0])
    at = np.flatnonzero(keep)
    rows = np.stack([x[at] for x in k + c], axis=1).astype(np.int32)
    return at.astype(np.int64), rows


def on_device(v):
    """a uint64 vector in HBM (as its int64 bits); at least one element so that the address is real"""
    a = np.ascontiguousarray(v, dtype=np.uint64)
    return torch.from_numpy(np.concatenate([a, np.zeros(2, dtype=np.uint64)]).view(np.int64)).cuda()


def run(eng, tested, controls, tables, W, capacity=None):
    dt, dc = [on_device(v) for v in tested], [on_device(v) for v in controls]
    got = eng.window_select([t.data_ptr() for t in dt], tables, W, controls=[t.data_ptr() for t in dc] if dc else None, n_windows=len(tested[0]),
                            capacity=capacity)
    torch.cuda.synchronize()
    return got


def check(eng, tested, controls, tables, W):
    at, rows = rule(tested, controls, tables, W)
    o, r, kept = run(eng, tested, controls, tables, W)
    assert kept == len(at)
    np.testing.assert_array_equal(o, at)
    np.testing.assert_array_equal(r, rows)
    return len(at)


def random_case(seed, n, nt, ctl, W, hi=None):
    rng = np.random.default_rng(seed)
    hi = hi or 2 * W
    tested = [rng.integers(0, hi + 1, size=n).astype(np.uint64) for _ in range(nt)]
    controls = [rng.integers(0, hi + 1, size=n).astype(np.uint64) for _ in range(nt)] if ctl else []
    # critical counts around the top of the clamped range: a fifth to a third of the windows kept
    tables = [rng.integers(W - W // 8, W + (2 if ctl else 1), size=W + 1 if ctl else 1).astype(np.int32) for _ in range(nt)]   # (W + 1: never reached)
    return tested, controls, tables


def test_limits_are_what_the_shapes_assume():
    assert TILE >= 128 and TILE % 128 == 0 and LDS_MAX_W >= 500
    assert 4 * (LDS_MAX_W + 1) * 4 == 64 * 1024                      # four tables of W + 1 int32 fill the LDS budget exactly


@pytest.mark.parametrize("nt,ctl", [(1, False), (1, True), (2, False), (2, True), (4, False), (4, True), (3, True)])
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_sizes_around_the_tile(eng, n, nt, ctl):
    tested, controls, tables = random_case(n * 10 + nt, n, nt, ctl, 20)
    kept = check(eng, tested, controls, tables, 20)
    assert n < TILE - 1 or 0 < kept < n


@pytest.mark.parametrize("ctl", [False, True])
def test_nothing_everything_last_tile_and_empty_runs(eng, ctl):
    n, W, nt = 6 * TILE + 5, 10, 2
    zeros = [np.zeros(n, dtype=np.uint64) for _ in range(nt)]
    controls = [np.full(n, 3, dtype=np.uint64) for _ in range(nt)] if ctl else []
    tables = [np.full(W + 1 if ctl else 1, 5, dtype=np.int32) for _ in range(nt)]
    assert check(eng, zeros, controls, tables, W) == 0                                          # nothing kept
    full = [np.full(n, 7, dtype=np.uint64) for _ in range(nt)]
    assert check(eng, full, controls, tables, W) == n                                           # everything kept
    never = [np.full(W + 1 if ctl else 1, W + 1, dtype=np.int32) for _ in range(nt)]
    assert check(eng, full, controls, never, W) == 0                                            # W + 1: no count reaches it
    last = [v.copy() for v in zeros]
    last[1][6 * TILE:] = 9
    assert check(eng, last, controls, tables, W) == 5                                           # kept windows only in the last, partial tile
    gaps = [v.copy() for v in zeros]
    gaps[0][[0, TILE - 1]] = 5; gaps[1][[4 * TILE, 4 * TILE + 1, 4 * TILE + 127, 4 * TILE + 128, 5 * TILE - 1]] = 6; gaps[0][n - 1] = 100
    assert check(eng, gaps, controls, tables, W) == 8                                           # tiles 1..3 and 5 empty between kept ones


def test_values_at_the_critical_count_and_one_below(eng):
    W, n = 50, TILE + 3
    rng = np.random.default_rng(5)
    tables = [rng.integers(1, W + 1, size=W + 1).astype(np.int32) for _ in range(2)]
    controls = [rng.integers(0, W + 30, size=n).astype(np.uint64) for _ in range(2)]              # c = 0 .. W and beyond
    controls[0][:4] = [0, W, W + 1, 2**40]; controls[1][:4] = [W, 0, 2**33, W + 7]
    crit = [tables[f][np.minimum(controls[f], np.uint64(W)).astype(np.int64)].astype(np.int64) for f in range(2)]
    at_crit = [crit[0].astype(np.uint64), (crit[1] - 1).astype(np.uint64)]                      # vector 0 exactly at its critical count: all kept
    assert check(eng, at_crit, controls, tables, W) == n
    below = [(crit[0] - 1).astype(np.uint64), (crit[1] - 1).astype(np.uint64)]                   # one below in both: none
    assert check(eng, below, controls, tables, W) == 0
    mixed = [np.where(np.arange(n) % 3 == 0, crit[0], crit[0] - 1).astype(np.uint64), np.where(np.arange(n) % 5 == 0, crit[1], crit[1] - 1).astype(np.uint64)]
    assert check(eng, mixed, controls, tables, W) == len(np.flatnonzero((np.arange(n) % 3 == 0) | (np.arange(n) % 5 == 0)))


def test_clamp_shows_in_the_rows_and_64_bit_values_are_compared_whole(eng):
    W, n = 12, 2 * TILE
    tested = [np.full(n, 3, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]
    tested[0][[1, 200, TILE + 1]] = [W + 1, 2**32, 2**63 + 5]        # low words 0 and 5: a 32-bit comparison would drop them
    tested[1][[7, TILE + 9]] = [2**32 + 1, 2**40]
    controls = [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]
    controls[0][[1, 5]] = [2**32, 2**35 + 2]                         # c > W clamps to W: the table's last entry
    tables = [np.full(W + 1, W, dtype=np.int32), np.full(W + 1, W, dtype=np.int32)]
    tables[0][W] = 3                                                  # under a control at or above W, 3 reads suffice
    o, r, kept = run(eng, tested, controls, tables, W)
    at, rows = rule(tested, controls, tables, W)
    assert at.tolist() == [1, 5, 7, 200, TILE + 1, TILE + 9]
    np.testing.assert_array_equal(o, at); np.testing.assert_array_equal(r, rows)
    assert r[0].tolist() == [W, 0, W, 0] and r[1].tolist() == [3, 0, W, 0] and r[2].tolist() == [3, W, 0, 0] and r.max() == W


def test_a_control_for_some_vectors_only_is_refused(eng):
    v = on_device(np.zeros(16, dtype=np.uint64))
    tab = [np.zeros(6, dtype=np.int32)] * 2
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        eng.window_select([v.data_ptr(), v.data_ptr()], tab, 5, controls=[v.data_ptr(), None], n_windows=16)
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        eng.window_select([v.data_ptr()] * 5, tab * 3, 5, n_windows=16)                         # five tested vectors
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        eng.window_select([v.data_ptr() + 8], tab[:1], 5, n_windows=8)                          # not 16-byte aligned
    o, r, kept = eng.window_select([v.data_ptr()], [np.ones(1, dtype=np.int32)], 5, controls=[None], n_windows=16)   # no control at all: fine
    assert kept == 0


@pytest.mark.parametrize("nt,W", [(4, LDS_MAX_W), (4, LDS_MAX_W + 1), (1, 4 * (LDS_MAX_W + 1) - 1), (1, 4 * (LDS_MAX_W + 1))],
                         ids=["lds_4", "global_4", "lds_1", "global_1"])
def test_window_size_at_the_table_path_switch(eng, nt, W):
    n = 2 * TILE + 3
    rng = np.random.default_rng(W + nt)
    tested = [rng.integers(0, W + 50, size=n).astype(np.uint64) for _ in range(nt)]
    controls = [rng.integers(0, W + 50, size=n).astype(np.uint64) for _ in range(nt)]
    for f in range(nt):
        controls[f][:3] = [0, W, W + 1]                              # the first and the last entry of every table are read
    tables = [rng.integers(W - W // 6, W + 2, size=W + 1).astype(np.int32) for _ in range(nt)]
    assert 0 < check(eng, tested, controls, tables, W) < n


def test_capacity_one_short_then_enough(eng):
    n, W = 3 * TILE + 7, 20
    tested, controls, tables = random_case(77, n, 2, True, W)
    at, rows = rule(tested, controls, tables, W)
    assert len(at) > TILE
    cap = len(at) - 1
    o, r, kept = run(eng, tested, controls, tables, W, capacity=cap)
    assert kept == len(at) and len(o) == cap                          # the needed count is reported
    np.testing.assert_array_equal(o, at[:cap]); np.testing.assert_array_equal(r, rows[:cap])
    # the device form: nothing is written past capacity
    dt, dc = [on_device(v) for v in tested], [on_device(v) for v in controls]
    d_o = torch.full((len(at) + 64,), -7, dtype=torch.int64, device="cuda")
    d_r = torch.full(((len(at) + 64) * 4,), -7, dtype=torch.int32, device="cuda")
    kept = eng.window_select([t.data_ptr() for t in dt], tables, W, controls=[t.data_ptr() for t in dc], n_windows=n, capacity=cap,
                             device_out=(d_o.data_ptr(), d_r.data_ptr()))
    torch.cuda.synchronize()
    assert kept == len(at)
    ho, hr = d_o.cpu().numpy(), d_r.cpu().numpy()
    np.testing.assert_array_equal(ho[:cap], at[:cap]); np.testing.assert_array_equal(hr[:cap * 4].reshape(cap, 4), rows[:cap])
    assert (ho[cap:] == -7).all() and (hr[cap * 4:] == -7).all()
    o, r, kept = run(eng, tested, controls, tables, W, capacity=kept)  # a second call with enough room is exact
    np.testing.assert_array_equal(o, at); np.testing.assert_array_equal(r, rows)
    assert run(eng, tested, controls, tables, W, capacity=0)[2] == len(at)


def test_two_calls_in_turn_on_one_context(eng):
    a = random_case(1, 2 * TILE + 1, 4, True, 30)
    b = random_case(2, TILE - 5, 1, False, 7)
    for _ in range(2):
        check(eng, *a, 30)
        check(eng, *b, 7)
