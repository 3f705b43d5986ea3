"""The tile prefix of the tile compactions (launch_tile_prefix: block_exclusive_sum, csrc/gtx_compact.h) with more tiles than its one
block has threads, through the peak candidate selection, whose inputs are the cheapest: 1024 threads, each over `per` consecutive
tiles, their counts loaded eight at a time.

    tiles   per
    1024    1     the last size with one tile per thread
    1025    2     the upper half of the threads without a tile
    8192    8     one full batch of loads
    8193    9     a batch and a tail

The signal is zero except in the first and the last window of the tiles on both sides of a seam between two threads' runs, of the
first tile and of the last, which is three windows short; the answer is those ordinals in order, each with the row (15, 0, 20)."""
import numpy as np
import pytest
import torch

import gtx

pytestmark = pytest.mark.gpu

T = gtx.PEAK_TILE
THREADS = 1024


@pytest.fixture(scope="module")
def eng():
    e = gtx.Engine(0)
    yield e
    e.close()


def marked_windows(nt, n):
    per = (nt + THREADS - 1) // THREADS
    tiles = {0, nt - 1}
    for k in (1, 2, 511, 512, 513, 1023):
        tiles |= {t for t in (k * per - 1, k * per) if 0 <= t < nt}
    return np.array(sorted({w for t in tiles for w in (t * T, min(t * T + T, n) - 1)}), dtype=np.int64), per


@pytest.mark.parametrize("nt", [1024, 1025, 8192, 8193])
def test_more_tiles_than_threads_in_the_tile_prefix(eng, nt):
    n = nt * T - 3
    want, per = marked_windows(nt, n)
    assert per == {1024: 1, 1025: 2, 8192: 8, 8193: 9}[nt] and want[0] == 0 and want[-1] == n - 1 and len(want) >= 8
    S = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    S[torch.from_numpy(want).cuda()] = 15
    C = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    o, r, kept = eng.peak_select(S.data_ptr(), C.data_ptr(), 20, 10, n_windows=n)
    torch.cuda.synchronize()
    assert kept == len(want)
    np.testing.assert_array_equal(o, want)
    np.testing.assert_array_equal(r, np.tile(np.array([15, 0, 20], dtype=np.int64), (len(want), 1)))
    # the device entry with room for half of them: the exact prefix, and nothing behind the capacity
    cap = len(want) // 2
    d_o = torch.full((len(want) + 64,), -7, dtype=torch.int64, device="cuda")
    d_r = torch.full((3 * (len(want) + 64),), -7, dtype=torch.int64, device="cuda")
    assert eng.peak_select_device(S.data_ptr(), C.data_ptr(), 20, 10, cap, d_o.data_ptr(), d_r.data_ptr(), n_windows=n) == len(want)
    torch.cuda.synchronize()
    ho, hr = d_o.cpu().numpy(), d_r.cpu().numpy()
    np.testing.assert_array_equal(ho[:cap], want[:cap])
    np.testing.assert_array_equal(hr[:3 * cap].reshape(-1, 3), np.tile(np.array([15, 0, 20], dtype=np.int64), (cap, 1)))
    assert (ho[cap:] == -7).all() and (hr[3 * cap:] == -7).all()
