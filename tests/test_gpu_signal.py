"""gtx_signal_bins / gtx_signal_bins_device (csrc/gtx_signal.hip) against a restatement of the reference's inner loop
(gtools/genomic_apps.cpp:560-605 heatmap, :826-880 profile): every overlapping (read, region) pair -- found here by brute force
over the regions' intervals, so independently of the device index -- adds its read's weight to the bin of the 5' offset of the
read's front interval, x / z / bin in IEEE doubles (the formulas of oracle/restate.py).  Weights are integers, so the sums do not depend on the order of the pairs."""
import numpy as np
import pytest

import gtx
from oracle.restate import offset_from, signal_bin

pytestmark = pytest.mark.gpu


def make_refs(rng, m, span, shift_up=5000, shift_down=5000, multi=0.0, n_chrom=3):
    """stranded regions, shifted as the reference shifts them (5' interval upstream, 3' interval downstream)"""
    regs = []
    for _ in range(m):
        c = int(rng.integers(0, n_chrom)); s = int(rng.integers(1, span)); minus = bool(rng.integers(0, 2))
        if rng.random() < multi:
            iv, at = [], s
            for _ in range(int(rng.integers(2, 5))):
                sz = int(rng.integers(5, 400)); iv.append([at, at + sz]); at += sz + int(rng.integers(30, 500))
        else:
            iv = [[s, s + int(rng.integers(0, 3000))]]
        if minus:
            iv[-1][1] += shift_up; iv[0][0] -= shift_down
        else:
            iv[0][0] -= shift_up; iv[-1][1] += shift_down
        regs.append((c, minus, [tuple(x) for x in iv]))
    return regs


def make_reads(rng, n, span, multi=0.0, zero=0.0, n_chrom=3, unknown=0.0):
    reads = []
    for _ in range(n):
        c = int(rng.integers(0, n_chrom)) if rng.random() >= unknown else n_chrom + 5
        s = int(rng.integers(1, span))
        if rng.random() < multi:
            iv, at = [], s
            for _ in range(int(rng.integers(2, 4))):
                sz = int(rng.integers(1, 100)); iv.append((at, at + sz)); at += sz + int(rng.integers(10, 300))
        elif rng.random() < zero:
            iv = [(s, s - 1)]
        else:
            iv = [(s, s + int(rng.integers(0, 300)))]
        reads.append((c, iv))
    return reads


def classes(c, minus, ignore):
    return c if ignore else 2 * c + int(minus)


def upload(e, regs, ignore):
    tri = np.array([(classes(c, m, ignore), iv[0][0], iv[-1][1]) for c, m, iv in regs], dtype=np.int32)
    e.set_refs(tri, 3 * (1 if ignore else 2) + 20)
    first = np.cumsum([0] + [len(iv) for _, _, iv in regs]).astype(np.int64)
    blocks = np.array([x for _, _, iv in regs for x in iv], dtype=np.int32)
    e.set_ref_blocks(first, blocks) if any(len(iv) > 1 for _, _, iv in regs) else e.set_ref_blocks(None)
    e.set_ref_strands(["-" if m else "+" for _, m, _ in regs])


def read_arrays(reads, strands, ignore):
    tri = np.array([(classes(c, st, ignore) if c < 3 else 99, iv[0][0], iv[-1][1]) for (c, iv), st in zip(reads, strands)], dtype=np.int32)
    multi = any(len(iv) > 1 for _, iv in reads)
    first = np.cumsum([0] + [len(iv) for _, iv in reads]).astype(np.int64) if multi else None
    blocks = np.array([x for _, iv in reads for x in iv], dtype=np.int32) if multi else None
    return tri, first, blocks


def expected(regs, reads, strands, weights, bin_min, bin_max, n_bins, per_ref, ref_len, ignore, zero_ok=False):
    out = np.zeros((len(regs) if per_ref else 1) * n_bins, dtype=np.int64)
    first_inv, dropped = -1, 0
    by_class = {}
    for k, (c, m, iv) in enumerate(regs):
        by_class.setdefault(classes(c, m, ignore), []).append(k)
    for i, ((c, iv), st) in enumerate(zip(reads, strands)):
        if c >= 3:
            continue
        s, e = iv[0][0], iv[-1][1]
        if s > e + (1 if zero_ok else 0):
            continue
        for k in by_class.get(classes(c, st, ignore), []):
            _, minus, riv = regs[k]
            if not (riv[0][0] <= e and riv[-1][1] >= s):
                continue
            if not any(a <= y and b >= x for a, b in riv for x, y in iv):
                continue
            a, b = offset_from(riv, minus, "5p", *iv[0])
            if a > b:
                first_inv = i if first_inv < 0 else first_inv
                continue
            j = signal_bin(a, b, 1 if ref_len is None else ref_len[k], bin_min, bin_max, n_bins)
            if j is None:
                continue
            if j >= n_bins:
                dropped += 1
                continue
            out[(k * n_bins if per_ref else 0) + j] += weights[i]
    return (out.reshape(len(regs), n_bins) if per_ref else out), first_inv, dropped


@pytest.fixture(scope="module")
def eng():
    e = gtx.Engine(0)
    yield e
    e.close()


CASES = [
    # name, per_ref, ignore, n_bins, ref multi, read multi, weighted, norm_ref_len, shuffled
    ("profile", False, False, 100, 0.0, 0.0, False, False, False),
    ("profile-i-weights", False, True, 100, 0.0, 0.0, True, False, True),
    ("profile-bed12", False, True, 64, 0.6, 0.3, True, False, False),
    ("profile-global-atomics", False, False, 9000, 0.0, 0.0, True, False, True),
    ("profile-norm-ref-len", False, True, 100, 0.3, 0.0, False, True, False),
    ("heatmap", True, False, 100, 0.0, 0.0, True, False, False),
    ("heatmap-i-bed12-shuffled", True, True, 40, 0.5, 0.3, True, False, True),
    ("heatmap-norm-ref-len", True, True, 333, 0.0, 0.0, True, True, True),
]


@pytest.mark.parametrize("name,per_ref,ignore,n_bins,rmulti,qmulti,weighted,norm,shuffled", CASES, ids=[c[0] for c in CASES])
def test_signal_bins_against_restatement(eng, name, per_ref, ignore, n_bins, rmulti, qmulti, weighted, norm, shuffled):
    rng = np.random.default_rng(sum(map(ord, name)))
    regs = make_refs(rng, 600, 400_000, multi=rmulti)
    reads = make_reads(rng, 30000, 400_000, multi=qmulti, unknown=0.02)
    if not shuffled:
        reads.sort(key=lambda r: (r[0], r[1][0][0]))
    strands = [bool(rng.integers(0, 2)) for _ in reads]
    weights = rng.integers(-4, 12, len(reads)).astype(np.int64) if weighted else np.ones(len(reads), dtype=np.int64)
    ref_len = [iv[-1][1] - iv[0][0] + 1 for _, _, iv in regs] if norm else None
    bin_min, bin_max = (0.0, 1.0) if norm else (-5000.0, 5000.0)
    upload(eng, regs, ignore)
    eng.set_signal_bins(bin_min, bin_max, n_bins, ref_len)
    tri, first, blocks = read_arrays(reads, strands, ignore)
    flags = gtx.SIGNAL_PER_REF if per_ref else 0
    want, winv, wdrop = expected(regs, reads, strands, weights, bin_min, bin_max, n_bins, per_ref, ref_len, ignore)
    got, inv, info = eng.signal_bins(tri, weights if weighted else None, flags, first, blocks)
    assert inv == winv == -1
    assert info["n_dropped"] == wdrop
    assert info["n_binned"] > 1000
    assert np.array_equal(got, want)
    if not weighted:
        assert info["weight_abs_sum"] == info["n_binned"] == int(want.sum())


def test_batches_and_device_entry(eng):
    """the host entry in batches of 1000 reads (GTX_BATCH_READS is read at creation: a second context) and the device entry
    on HBM-resident reads give the same bins"""
    import os
    import torch
    rng = np.random.default_rng(11)
    regs = make_refs(rng, 500, 300_000)
    reads = make_reads(rng, 20000, 300_000)
    reads.sort(key=lambda r: (r[0], r[1][0][0]))
    strands = [bool(rng.integers(0, 2)) for _ in reads]
    weights = rng.integers(0, 7, len(reads)).astype(np.int64)
    tri, _, _ = read_arrays(reads, strands, False)
    for per_ref in (False, True):
        want, _, _ = expected(regs, reads, strands, weights, -5000.0, 5000.0, 100, per_ref, None, False)
        os.environ["GTX_BATCH_READS"] = "1000"
        try:
            e2 = gtx.Engine(0)
        finally:
            del os.environ["GTX_BATCH_READS"]
        upload(e2, regs, False)
        e2.set_signal_bins(-5000.0, 5000.0, 100)
        got, inv, _ = e2.signal_bins(tri, weights, gtx.SIGNAL_PER_REF if per_ref else 0)
        e2.close()
        assert inv == -1 and np.array_equal(got, want)
        upload(eng, regs, False)
        eng.set_signal_bins(-5000.0, 5000.0, 100)
        d_tri = torch.from_numpy(tri.copy()).to("cuda:0")
        d_w = torch.from_numpy(weights).to("cuda:0")
        d_bins = torch.zeros(want.size, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        inv, info = eng.signal_bins_device(d_tri.data_ptr(), len(reads), d_bins.data_ptr(), d_w.data_ptr(), gtx.SIGNAL_PER_REF if per_ref else 0)
        assert inv == -1 and np.array_equal(d_bins.cpu().numpy(), want.reshape(-1))
        # called again the device entry adds to d_bins
        eng.signal_bins_device(d_tri.data_ptr(), len(reads), d_bins.data_ptr(), d_w.data_ptr(), gtx.SIGNAL_PER_REF if per_ref else 0)
        assert np.array_equal(d_bins.cpu().numpy(), 2 * want.reshape(-1))


def test_near_position_one_zero_length_and_inverted(eng):
    """regions shifted past position 1 (starts <= 0), zero-length reads (no pairs without GTX_ZERO_LENGTH_OK; with it their
    offsets are inverted: the first such read is reported and nothing of it is binned), reads of unknown classes"""
    regs = [(0, False, [(1 - 5000, 300 + 5000)]), (0, True, [(50 - 5000, 80 + 5000)]), (1, False, [(-4990, 5100)])]
    reads = [(0, [(10, 40)]), (0, [(60, 59)]), (0, [(200, 260)]), (5, [(10, 20)]), (1, [(1, 1)]), (0, [(70, 69)])]
    strands = [False, False, False, False, False, True]
    weights = np.array([1, 2, 3, 4, 5, 6], dtype=np.int64)
    upload(eng, regs, True)
    eng.set_signal_bins(-5000.0, 5000.0, 100)
    tri, _, _ = read_arrays(reads, strands, True)
    tri[3, 0] = 77
    want, _, _ = expected(regs, reads, strands, weights, -5000.0, 5000.0, 100, False, None, True)
    got, inv, info = eng.signal_bins(tri, weights, 0)
    assert inv == -1 and np.array_equal(got, want) and want.sum() > 0
    assert info["n_degenerate"] == 2 and info["n_no_class"] == 1
    got, inv, info = eng.signal_bins(tri, weights, gtx.ZERO_LENGTH_OK)
    assert inv == 1 and np.array_equal(got, want)


def test_call_order_errors(eng):
    regs = [(0, False, [(100, 200)])]
    upload(eng, regs, True)
    with pytest.raises(gtx.GtxError):
        eng.signal_bins(np.array([[0, 100, 150]], dtype=np.int32))          # no gtx_set_signal_bins since gtx_set_refs
    with pytest.raises(gtx.GtxError):
        eng.set_signal_bins(0.0, 1.0, -1)
