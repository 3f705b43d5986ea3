"""Scan results that stay on the device (gtx_scan_end_keep / gtx_scan_kept / gtx_scan_drop): a kept slot holds what Engine.scan
returns for the same reads, a later scan on the context leaves it alone, and a kept slot feeds the window selection."""
import ctypes

import numpy as np
import pytest

import gtx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = gtx.Engine(0)
    yield e
    e.close()


def read_back(addr, n):
    """n uint64 at a device address the library owns, copied by the HIP runtime the process already has"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(max(n, 1), dtype=np.uint64)
    assert hip.hipMemcpy(out.ctypes.data, addr, n * 8, 2) == 0       # device to host
    return out[:n]


CLASS_LEN = np.array([200000, 150001, 99999, 499], dtype=np.int64)  # (the last class is shorter than a window: no windows)


def reads(n, seed, shuffle=False):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 3, size=n)
    start = (rng.random(n) ** 2 * (CLASS_LEN[cls] - 60)).astype(np.int64) + 1        # denser towards the front
    a = np.stack([cls, start, start + 49], axis=1)
    a = a[rng.permutation(n)] if shuffle else a[np.lexsort((a[:, 1], a[:, 0]))]
    return a.astype(np.int32)


def test_kept_slots_equal_the_scan_and_survive_a_later_scan(eng):
    a, b = reads(40000, 3), reads(25000, 4, shuffle=True)
    wa, off = eng.scan(a, CLASS_LEN, 100, 500, preprocess="c")
    wb, _ = eng.scan(b, CLASS_LEN, 100, 500, preprocess="c", flags=gtx.READS_UNSORTED)
    pa, na, off2 = eng.scan_keep(0, a, CLASS_LEN, 100, 500, preprocess="c")
    pb, nb, _ = eng.scan_keep(5, b, CLASS_LEN, 100, 500, preprocess="c", flags=gtx.READS_UNSORTED)
    assert (na, nb) == (len(wa), len(wb)) and pa != pb and pa % 16 == 0 and pb % 16 == 0
    np.testing.assert_array_equal(off, off2)
    np.testing.assert_array_equal(read_back(pa, na), wa)
    np.testing.assert_array_equal(read_back(pb, nb), wb)
    other, _ = eng.scan(b, CLASS_LEN, 1000, 1000)                    # a plain scan, another geometry
    assert other.sum() > 0
    assert eng.scan_kept(0) == (pa, na) and eng.scan_kept(5) == (pb, nb)
    np.testing.assert_array_equal(read_back(pa, na), wa)
    np.testing.assert_array_equal(read_back(pb, nb), wb)
    # the kept slots feed the selection: the windows in the top tenth of either input
    ta, tb = int(np.quantile(wa, 0.9)) + 1, int(np.quantile(wb, 0.9)) + 1
    o, r, kept = eng.window_select([0, 5], [np.array([ta], dtype=np.int32), np.array([tb], dtype=np.int32)], 500)
    want = np.flatnonzero((wa >= ta) | (wb >= tb))
    assert 0 < kept == len(want) < na
    np.testing.assert_array_equal(o, want)
    np.testing.assert_array_equal(r, np.stack([np.minimum(wa, 500)[want], np.minimum(wb, 500)[want]], axis=1).astype(np.int32))


def test_a_slot_is_replaced_and_dropped(eng):
    a = reads(5000, 9)
    w1, _ = eng.scan(a, CLASS_LEN, 1000, 1000)
    p1, n1, _ = eng.scan_keep(2, a, CLASS_LEN, 1000, 1000)
    np.testing.assert_array_equal(read_back(p1, n1), w1)
    w2, _ = eng.scan(a, CLASS_LEN[:3], 500, 1000)               # another geometry in the same slot
    p2, n2, _ = eng.scan_keep(2, a[a[:, 0] < 3], CLASS_LEN[:3], 500, 1000)
    assert n2 == len(w2) != n1
    np.testing.assert_array_equal(read_back(p2, n2), w2)
    eng.scan_drop(2)
    with pytest.raises(gtx.GtxError, match="gtx error -3"):
        eng.scan_kept(2)
    eng.scan_keep(1, a, CLASS_LEN, 1000, 1000); eng.scan_keep(7, a, CLASS_LEN, 1000, 1000)
    eng.scan_drop()                                                  # -1: all of them
    for slot in (1, 7):
        with pytest.raises(gtx.GtxError, match="gtx error -3"):
            eng.scan_kept(slot)
    w3, _ = eng.scan(a, CLASS_LEN, 1000, 1000)                  # the context still scans
    np.testing.assert_array_equal(w3, w1)


def test_slot_8_is_refused(eng):
    a = reads(100, 1)
    for slot in (8, -1):
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            eng.scan_keep(slot, a, CLASS_LEN, 1000, 1000)
        w, _ = eng.scan(a, CLASS_LEN, 1000, 1000)              # the refused call left no scan open
        assert 0 < w.sum() <= 100
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        eng.scan_kept(8)
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        eng.scan_drop(8)
    assert eng.lib.gtx_scan_end_keep(eng.ctx, 0, None) == -3         # no scan is open
