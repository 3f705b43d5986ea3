"""The overlap join (gtx_join / gtx_join_device, include/gtx.h; kernels in csrc/gtx_join.hip): every (query, reference region)
pair that overlaps, grouped by query, and within a query in the reference's iteration order -- ascending ordinal for the sorted
merge, (level, bin, -ordinal) for the bin index.  Expected values: the oracle's `pairs` operation (oracle/gtx_oracle.c), which
prints `<query line>\t<reference label>` per pair in the order GetOverlap / NextOverlap deliver them, on BED files written from
the same arrays."""
import os
import subprocess

import numpy as np
import pytest

import gtx
from oracle import orc
from oracle.restate import NAMES, bin_keys, concat, multi, regions, take, triples, write_bed

pytestmark = pytest.mark.gpu


def oracle_rows(tmp, args):
    r = subprocess.run([orc.CLI, "pairs"] + args + ["refs.bed", "reads.bed"], capture_output=True, cwd=tmp)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode().splitlines()


def join_rows(off, pairs):
    rows = []
    for i in range(len(off) - 1):
        rows += ["%d\tr%d" % (i + 1, k) for k in pairs[off[i]:off[i + 1]]]
    return rows


def run(engine, tmp, refs, reads, sorted_=False, ign=True, gaps=False, bits=None, by_strand=False, buffer=None, capacity=None):
    write_bed(tmp / "refs.bed", refs, "r")
    write_bed(tmp / "reads.bed", reads, "q")
    args = (["-S"] if sorted_ else []) + (["-s"] if by_strand else []) + (["-i"] if ign else []) + (["-gaps"] if gaps else []) + \
           (["-B", bits] if bits else [])
    want = oracle_rows(tmp, args)
    n_classes = len(NAMES) * (1 if ign else 2)
    engine.set_refs(triples(refs, ign), n_classes, gtx.REFS_KEEP_ZERO_LENGTH if sorted_ else 0)
    mr = multi(refs)
    engine.set_ref_blocks(*mr) if mr else engine.set_ref_blocks(None)
    engine.set_ref_order(None if sorted_ else bin_keys(refs, bits or "17,20,23,26"))
    engine.set_join_buffer(buffer or (1 << 26))
    mq = multi(reads)
    flags = (gtx.ZERO_LENGTH_OK if sorted_ else 0) | (gtx.JOIN_GAPS if gaps else 0)
    off, pairs, info = engine.join(triples(reads, ign), flags, *(mq or (None, None)), capacity=capacity)
    return want, off, pairs, info


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(2026)


CASES = [
    # name, refs kwargs, reads kwargs, run kwargs
    ("bin_default", dict(n=3000, span=400_000, lmin=1, lmax=4000), dict(n=20_000, span=400_000, lmin=1, lmax=300), dict()),
    ("bin_strand", dict(n=3000, span=400_000, lmin=1, lmax=4000), dict(n=20_000, span=400_000, lmin=1, lmax=300), dict(ign=False)),
    ("bin_levels", dict(n=2000, span=3_000_000, lmin=1, lmax=3000, wide=60), dict(n=6000, span=3_000_000, lmin=1, lmax=200_000),
     dict(bits="10,14,18")),
    ("bin_wide_default", dict(n=2000, span=3_000_000, lmin=1, lmax=3000, wide=60), dict(n=6000, span=3_000_000, lmin=1, lmax=200_000), dict()),
    ("bin_shuffled", dict(n=3000, span=400_000, lmin=1, lmax=4000, sort="none"), dict(n=20_000, span=400_000, lmin=1, lmax=300, sort="none"),
     dict()),
    ("merge", dict(n=3000, span=400_000, lmin=1, lmax=4000), dict(n=20_000, span=400_000, lmin=1, lmax=300), dict(sorted_=True)),
    ("merge_strand", dict(n=3000, span=400_000, lmin=1, lmax=4000), dict(n=20_000, span=400_000, lmin=1, lmax=300),
     dict(sorted_=True, ign=False)),
    ("merge_by_strand", dict(n=3000, span=400_000, lmin=1, lmax=4000, sort="strand"), dict(n=20_000, span=400_000, lmin=1, lmax=300, sort="strand"),
     dict(sorted_=True, ign=False, by_strand=True)),
    ("merge_wide", dict(n=2000, span=3_000_000, lmin=1, lmax=3000, wide=60), dict(n=6000, span=3_000_000, lmin=1, lmax=200_000),
     dict(sorted_=True)),
    ("bed12", dict(n=2000, span=300_000, lmin=1, lmax=3000, multi=0.6), dict(n=8000, span=300_000, lmin=1, lmax=200, multi=0.3), dict()),
    ("bed12_gaps", dict(n=2000, span=300_000, lmin=1, lmax=3000, multi=0.6), dict(n=8000, span=300_000, lmin=1, lmax=200, multi=0.3),
     dict(gaps=True)),
    ("bed12_merge", dict(n=2000, span=300_000, lmin=1, lmax=3000, multi=0.6), dict(n=8000, span=300_000, lmin=1, lmax=200, multi=0.3),
     dict(sorted_=True)),
    ("bed12_merge_gaps", dict(n=2000, span=300_000, lmin=1, lmax=3000, multi=0.6), dict(n=8000, span=300_000, lmin=1, lmax=200, multi=0.3),
     dict(sorted_=True, gaps=True)),
    ("bin_split", dict(n=3000, span=400_000, lmin=1, lmax=4000), dict(n=20_000, span=400_000, lmin=1, lmax=3000), dict(buffer=777)),
    ("merge_split", dict(n=3000, span=400_000, lmin=1, lmax=4000), dict(n=20_000, span=400_000, lmin=1, lmax=3000), dict(sorted_=True, buffer=500)),
]


@pytest.mark.parametrize("name,rk,qk,kw", CASES, ids=[c[0] for c in CASES])
def test_join_equals_the_oracle_pairs(engine, rng, tmp_path, name, rk, qk, kw):
    refs, reads = regions(rng, **rk), regions(rng, **qk)
    want, off, pairs, info = run(engine, tmp_path, refs, reads, **kw)
    assert len(want) > 1000                                                    # the fixture is not vacuous
    assert join_rows(off, pairs) == want
    assert info["n_no_class"] == 0 and info["n_degenerate"] == 0


def test_unknown_chromosomes_match_nothing(engine, rng, tmp_path):
    refs = regions(rng, 2000, 300_000, 1, 3000, n_chrom=2)
    reads = regions(rng, 10_000, 300_000, 1, 300, n_chrom=3)                   # chr3: not in the reference set
    want, off, pairs, info = run(engine, tmp_path, refs, reads)
    assert join_rows(off, pairs) == want and len(want) > 1000
    assert np.diff(off)[reads["chrom"] == 2].sum() == 0 and (reads["chrom"] == 2).sum() > 0
    off_u, _, info_u = engine.join(triples(reads, True, n_known=2))            # chr3 as a class outside [0, n_classes)
    assert np.array_equal(off_u, off) and info_u["n_no_class"] == int((reads["chrom"] == 2).sum())
    off_s, pairs_s, _ = run(engine, tmp_path, refs, reads, sorted_=True)[1:]
    assert join_rows(off_s, pairs_s) == oracle_rows(tmp_path, ["-S", "-i"])


def test_zero_length_and_inverted_under_the_merge(engine, rng, tmp_path):
    """-S: the merge never validates; zero-length (BED start == end) and inverted (start > end) intervals match by the two
    comparisons of CalcDirection on both sides"""
    refs = regions(rng, 3000, 200_000, 1, 2000)
    reads = regions(rng, 15_000, 200_000, 1, 200)
    for r, frac in ((refs, 0.1), (reads, 0.1)):
        n = len(r["s"])
        z = rng.random(n) < frac
        r["e"][z] = r["s"][z] - 1                                               # zero length
        inv = (rng.random(n) < frac) & ~z
        r["e"][inv] = r["s"][inv] - rng.integers(2, 50, size=int(inv.sum()))    # inverted
        r["blocks"][:, 1] = r["e"]
    want, off, pairs, info = run(engine, tmp_path, refs, reads, sorted_=True)
    assert join_rows(off, pairs) == want and len(want) > 1000
    assert info["n_degenerate"] > 0                                            # inverted queries are reported, and still matched


def test_long_walks_and_big_segments(engine, rng, tmp_path):
    """one query over more than 10 000 regions, one region under more than 10 000 queries; both orders; the big query alone
    exceeds the join buffer"""
    refs = regions(rng, 30_000, 2_000_000, 1, 300, n_chrom=1)
    refs = concat(refs, dict(chrom=np.array([0]), strand=np.array([0]), s=np.array([5]), e=np.array([1_999_000]),
                             first=np.array([0, 1]), blocks=np.array([[5, 1_999_000]])))          # under every query
    refs = take(refs, np.lexsort((refs["s"], refs["chrom"])))
    reads = regions(rng, 15_000, 2_000_000, 1, 100, n_chrom=1)
    big = dict(chrom=np.array([0]), strand=np.array([0]), s=np.array([10]), e=np.array([1_900_000]), first=np.array([0, 1]),
               blocks=np.array([[10, 1_900_000]]))
    reads = take(concat(reads, big), np.lexsort((concat(reads, big)["s"], concat(reads, big)["chrom"])))
    for sorted_ in (False, True):
        want, off, pairs, _ = run(engine, tmp_path, refs, reads, sorted_=sorted_, buffer=8000)
        seg = np.diff(off)
        assert seg.max() > 10_000
        assert join_rows(off, pairs) == want
        assert (pairs == np.flatnonzero(refs["e"] - refs["s"] > 1_000_000)[0]).sum() > 10_000


def test_pairs_beyond_the_capacity_are_cut_but_offsets_are_whole(engine, rng, tmp_path):
    refs, reads = regions(rng, 2000, 300_000, 1, 3000), regions(rng, 10_000, 300_000, 1, 300)
    want, off, pairs, _ = run(engine, tmp_path, refs, reads, capacity=1234, buffer=300)
    full = [int(x.split("\tr")[1]) for x in want]
    assert off[-1] == len(full) and list(pairs) == full[:1234]


def test_join_device(engine, rng, tmp_path):
    torch = pytest.importorskip("torch")
    refs, reads = regions(rng, 3000, 400_000, 1, 4000), regions(rng, 20_000, 400_000, 1, 300)
    want, off, pairs, _ = run(engine, tmp_path, refs, reads, sorted_=True)
    d_reads = torch.from_numpy(triples(reads, True)).cuda()
    d_off = torch.zeros(len(off), dtype=torch.int64, device="cuda")
    cap = int(off[len(off) // 2])                                             # room for the first half of the queries
    d_pairs = torch.zeros(cap, dtype=torch.int32, device="cuda")
    total, done, info = engine.join_device(d_reads.data_ptr(), len(off) - 1, d_off.data_ptr(), d_pairs.data_ptr(), cap, gtx.ZERO_LENGTH_OK)
    assert total == off[-1] and np.array_equal(d_off.cpu().numpy(), off)
    assert off[done] <= cap < off[done + 1] if done < len(off) - 1 else True
    assert np.array_equal(d_pairs.cpu().numpy()[:off[done]], pairs[:off[done]])
    assert info["n_no_class"] == 0


def test_join_device_sorts_bin_order_segments(engine, rng, tmp_path):
    """gtx_join_device with bin-index keys: the segment sort (and its scratch) behind the device entry"""
    torch = pytest.importorskip("torch")
    refs = regions(rng, 2000, 3_000_000, 1, 3000, wide=60)
    reads = regions(rng, 6000, 3_000_000, 1, 200_000)
    want, off, pairs, _ = run(engine, tmp_path, refs, reads)
    assert np.diff(off).max() > 32                                           # segments the block sort takes
    d_reads = torch.from_numpy(triples(reads, True)).cuda()
    d_off = torch.zeros(len(off), dtype=torch.int64, device="cuda")
    d_pairs = torch.zeros(int(off[-1]), dtype=torch.int32, device="cuda")
    total, done, _ = engine.join_device(d_reads.data_ptr(), len(off) - 1, d_off.data_ptr(), d_pairs.data_ptr(), int(off[-1]))
    assert total == off[-1] and done == len(off) - 1
    assert join_rows(d_off.cpu().numpy(), d_pairs.cpu().numpy()) == want


def test_check_sorted_reports_the_first_violation_across_batches(engine, rng, tmp_path):
    """GTX_CHECK_SORTED: a violation at the seam between two host batches comes before one inside the second batch"""
    refs, reads = regions(rng, 2000, 300_000, 1, 3000), regions(rng, 5000, 300_000, 1, 300)
    run(engine, tmp_path, refs, reads, sorted_=True)
    t = triples(reads, True)
    t[4000] = t[0]                                                          # inside the second batch of 3000
    t[3000, 0] = 0; t[3000, 1] = 1                                          # at the seam
    old = os.environ.get("GTX_BATCH_READS")
    os.environ["GTX_BATCH_READS"] = "3000"                                  # (read when a context is made)
    try:
        e = gtx.Engine(0)
    finally:
        if old is None:
            del os.environ["GTX_BATCH_READS"]
        else:
            os.environ["GTX_BATCH_READS"] = old
    try:
        e.set_refs(triples(refs, True), len(NAMES), gtx.REFS_KEEP_ZERO_LENGTH)
        off, _, info = e.join(t, gtx.ZERO_LENGTH_OK | gtx.CHECK_SORTED)
        assert info["first_unsorted"] == 3000
        off_all, _, info_all = engine.join(t, gtx.ZERO_LENGTH_OK | gtx.CHECK_SORTED)
        assert info_all["first_unsorted"] == 3000 and np.array_equal(off, off_all)
    finally:
        e.close()
