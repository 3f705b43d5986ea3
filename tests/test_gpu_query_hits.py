"""Per-query hits (gtx_query_hits / gtx_query_hits_device, include/gtx.h; kernels in csrc/gtx_query.hip): for every query the
number of reference regions it overlaps.  Expected values: column 2 of the oracle's `qstats` operation (oracle/gtx_oracle.c: the
reference's CountQueryOverlaps per query line, `--max-label-value 1`, so the pair count) on BED files written from the same
arrays.  Every case is also held to the lengths of gtx_join's segments and to the join's info; the cases that differ in what
the walk has to look at -- interval lists on either side, -gaps, zero-length and inverted intervals under the merge -- assert the
quantity that makes the difference."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gtx
from oracle import orc
from oracle.restate import NAMES, bin_keys, concat, multi, regions, take, triples, write_bed

pytestmark = pytest.mark.gpu

OK, E_ARG, E_STATE = 0, -1, -3                                              # include/gtx.h


def oracle_hits(tmp, args, n):
    r = subprocess.run([orc.CLI, "qstats"] + args + ["refs.bed", "reads.bed"], capture_output=True, cwd=tmp)
    assert r.returncode == 0, r.stderr.decode()
    rows = [x.split("\t") for x in r.stdout.decode().splitlines()]
    assert [int(x[0]) for x in rows] == list(range(1, n + 1))                   # one row per query line, in order
    return np.array([int(x[1]) for x in rows], dtype=np.uint32)


def setup(engine, tmp, refs, reads, sorted_=False, ign=True, gaps=False, bits=None, by_strand=False):
    """the reference set on the engine as test_gpu_join.run sets it; (oracle's hits, query triples, interval lists, flags)"""
    write_bed(tmp / "refs.bed", refs, "r")
    write_bed(tmp / "reads.bed", reads, "q")
    args = (["-S"] if sorted_ else []) + (["-s"] if by_strand else []) + (["-i"] if ign else []) + (["-gaps"] if gaps else []) + \
           (["-B", bits] if bits else [])
    want = oracle_hits(tmp, args, len(reads["s"]))
    engine.set_refs(triples(refs, ign), len(NAMES) * (1 if ign else 2), gtx.REFS_KEEP_ZERO_LENGTH if sorted_ else 0)
    mr = multi(refs)
    engine.set_ref_blocks(*mr) if mr else engine.set_ref_blocks(None)
    engine.set_ref_order(None if sorted_ else bin_keys(refs, bits or "17,20,23,26"))
    flags = (gtx.ZERO_LENGTH_OK if sorted_ else 0) | (gtx.JOIN_GAPS if gaps else 0)
    return want, triples(reads, ign), multi(reads) or (None, None), flags


def check(engine, tmp, refs, reads, **kw):
    """hits == the oracle's == the join's segment lengths, with the join's info; returns (hits, info)"""
    want, tri, mq, flags = setup(engine, tmp, refs, reads, **kw)
    hits, info = engine.query_hits(tri, flags, *mq)
    off, _, jinfo = engine.join(tri, flags, *mq, capacity=0)
    assert hits.dtype == np.uint32 and np.array_equal(hits, want)
    assert np.array_equal(hits, np.diff(off))
    assert info == jinfo
    return hits, info


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(2027)


R = dict(n=3000, span=400_000, lmin=1, lmax=4000)
Q = dict(n=20_000, span=400_000, lmin=1, lmax=300)
RW = dict(n=2000, span=3_000_000, lmin=1, lmax=3000, wide=60)
QW = dict(n=6000, span=3_000_000, lmin=1, lmax=200_000)
R12 = dict(n=2000, span=300_000, lmin=1, lmax=3000, multi=0.6)
Q12 = dict(n=8000, span=300_000, lmin=1, lmax=200, multi=0.3)

CASES = [
    # name, refs kwargs, reads kwargs, run kwargs
    ("bin_default", R, Q, dict()),
    ("bin_strand", R, Q, dict(ign=False)),
    ("bin_levels", RW, QW, dict(bits="10,14,18")),
    ("bin_shuffled", dict(R, sort="none"), dict(Q, sort="none"), dict()),
    ("merge", R, Q, dict(sorted_=True)),
    ("merge_strand", R, Q, dict(sorted_=True, ign=False)),
    ("merge_by_strand", dict(R, sort="strand"), dict(Q, sort="strand"), dict(sorted_=True, ign=False, by_strand=True)),
    ("merge_wide", RW, QW, dict(sorted_=True)),
    ("bed12", R12, Q12, dict()),
    ("bed12_gaps", R12, Q12, dict(gaps=True)),
    ("bed12_merge", R12, Q12, dict(sorted_=True)),
    ("bed12_merge_gaps", R12, Q12, dict(sorted_=True, gaps=True)),
    ("bed12_refs_only", R12, dict(Q12, multi=0.0), dict()),
    ("bed12_refs_only_gaps", R12, dict(Q12, multi=0.0), dict(gaps=True)),
    ("bed12_reads_only", dict(R12, multi=0.0), Q12, dict()),
    ("bed12_reads_only_gaps", dict(R12, multi=0.0), Q12, dict(gaps=True)),
]


@pytest.mark.parametrize("name,rk,qk,kw", CASES, ids=[c[0] for c in CASES])
def test_hits_equal_the_oracle_and_the_join(engine, rng, tmp_path, name, rk, qk, kw):
    refs, reads = regions(rng, **rk), regions(rng, **qk)
    # interval lists on the reference side and on the query side: which this case has
    assert (multi(refs) is not None) == (rk.get("multi", 0) > 0) and (multi(reads) is not None) == (qk.get("multi", 0) > 0)
    hits, info = check(engine, tmp_path, refs, reads, **kw)
    assert hits.sum() > 1000 and len(np.unique(hits)) > 3 and (hits == 0).any()   # the fixture is not vacuous
    assert info["n_no_class"] == 0 and info["n_degenerate"] == 0


def test_unknown_chromosomes_have_no_hits(engine, rng, tmp_path):
    refs = regions(rng, 2000, 300_000, 1, 3000, n_chrom=2)
    reads = regions(rng, 10_000, 300_000, 1, 300, n_chrom=3)                   # chr3: not in the reference set
    hits, info = check(engine, tmp_path, refs, reads)
    assert hits[reads["chrom"] == 2].sum() == 0 and (reads["chrom"] == 2).sum() > 0 and hits.sum() > 1000
    hits_u, info_u = engine.query_hits(triples(reads, True, n_known=2))        # chr3 as a class outside [0, n_classes)
    assert np.array_equal(hits_u, hits) and info_u["n_no_class"] == int((reads["chrom"] == 2).sum())
    t = triples(reads, True)
    t[::7, 0] = -1                                                             # class -1: nothing, and counted
    hits_m, info_m = engine.query_hits(t)
    assert hits_m[::7].sum() == 0 and np.array_equal(np.delete(hits_m, np.s_[::7]), np.delete(hits, np.s_[::7]))
    assert info_m["n_no_class"] == len(t[::7])
    check(engine, tmp_path, refs, reads, sorted_=True)


def test_nested_and_chromosome_spanning_regions(engine, rng, tmp_path):
    """one region under every query of its chromosome, one query over every region; regions nested in regions"""
    refs = regions(rng, 30_000, 2_000_000, 1, 300, n_chrom=1)
    nest = regions(rng, 3000, 2_000_000, 5000, 50_000, n_chrom=1)
    allr = dict(chrom=np.array([0]), strand=np.array([0]), s=np.array([5]), e=np.array([1_999_000]), first=np.array([0, 1]),
                blocks=np.array([[5, 1_999_000]]))
    refs = concat(concat(refs, nest), allr)
    refs = take(refs, np.lexsort((refs["s"], refs["chrom"])))
    reads = regions(rng, 15_000, 2_000_000, 1, 100, n_chrom=1)
    big = dict(chrom=np.array([0]), strand=np.array([0]), s=np.array([10]), e=np.array([1_900_000]), first=np.array([0, 1]),
               blocks=np.array([[10, 1_900_000]]))
    reads = concat(reads, big)
    reads = take(reads, np.lexsort((reads["s"], reads["chrom"])))
    for sorted_ in (False, True):
        hits, _ = check(engine, tmp_path, refs, reads, sorted_=sorted_)
        assert hits.max() > 30_000 and (hits >= 1).mean() > 0.99


def test_piles_on_one_position(engine, rng, tmp_path):
    """thousands of boundaries in one cell of the placement table: 5000 regions that start at one position, 4000 that end at
    one, among ordinary ones; queries on, before and behind the piles"""
    base = regions(rng, 4000, 1_000_000, 1, 2000, n_chrom=2)
    n1, n2 = 5000, 4000
    p1s = np.full(n1, 300_000); p1e = p1s + rng.integers(0, 3000, size=n1)
    p2e = np.full(n2, 700_000); p2s = p2e - rng.integers(0, 3000, size=n2)
    s, e = np.concatenate((p1s, p2s)), np.concatenate((p1e, p2e))
    pile = dict(chrom=np.zeros(n1 + n2, dtype=np.int64), strand=rng.integers(0, 2, size=n1 + n2), s=s, e=e,
                first=np.arange(n1 + n2 + 1, dtype=np.int64), blocks=np.stack([s, e], axis=1))
    refs = concat(base, pile)
    refs = take(refs, np.lexsort((refs["s"], refs["chrom"])))
    reads = regions(rng, 12_000, 1_000_000, 1, 300, n_chrom=2)
    m = 6000
    at = np.concatenate((rng.integers(296_000, 304_000, size=m // 2), rng.integers(696_000, 704_000, size=m // 2)))
    near = dict(chrom=np.zeros(m, dtype=np.int64), strand=rng.integers(0, 2, size=m), s=at, e=at + rng.integers(0, 50, size=m),
                first=np.arange(m + 1, dtype=np.int64), blocks=None)
    near["blocks"] = np.stack([near["s"], near["e"]], axis=1)
    edge = np.array([299_999, 300_000, 300_001, 699_999, 700_000, 700_001])
    one = dict(chrom=np.zeros(6, dtype=np.int64), strand=np.zeros(6, dtype=np.int64), s=edge, e=edge, first=np.arange(7, dtype=np.int64),
               blocks=np.stack([edge, edge], axis=1))
    reads = concat(concat(reads, near), one)
    reads = take(reads, np.lexsort((reads["s"], reads["chrom"])))
    for kw in (dict(), dict(ign=False), dict(sorted_=True)):
        hits, _ = check(engine, tmp_path, refs, reads, **kw)
        assert hits.max() >= (n1 if kw.get("ign", True) else n1 // 3)


def degenerate(rng, r, zero, inverted):
    """a fraction of r made zero-length (BED start == end) / inverted (start > end)"""
    n = len(r["s"])
    z = rng.random(n) < zero
    r["e"][z] = r["s"][z] - 1
    inv = (rng.random(n) < inverted) & ~z
    r["e"][inv] = r["s"][inv] - rng.integers(2, 50, size=int(inv.sum()))
    r["blocks"][:, 1] = r["e"]
    return int(z.sum()), int(inv.sum())


# -S: the merge never validates; zero-length and inverted intervals match by the two comparisons of CalcDirection on both sides.
MERGE_ODD = [
    # name, (zero, inverted) share of the regions, of the queries
    ("plain", (0, 0), (0, 0)),
    ("zero_refs", (0.1, 0), (0, 0)),                    # zero-length regions: start == stop + 1 stays inside the identity
    ("inverted_refs", (0.1, 0.1), (0, 0)),              # ... inverted ones do not
    ("zero_queries", (0.1, 0), (0.1, 0)),               # ... nor zero-length queries
    ("inverted_queries", (0, 0), (0, 0.1)),
    ("all", (0.1, 0.1), (0.1, 0.1)),
]


@pytest.mark.parametrize("name,rz,qz", MERGE_ODD, ids=[c[0] for c in MERGE_ODD])
def test_zero_length_and_inverted_under_the_merge(engine, rng, tmp_path, name, rz, qz):
    refs, reads = regions(rng, 3000, 200_000, 1, 2000), regions(rng, 15_000, 200_000, 1, 200)
    nrz, nri = degenerate(rng, refs, *rz)
    nqz, nqi = degenerate(rng, reads, *qz)
    assert (nrz > 0, nri > 0, nqz > 0, nqi > 0) == (rz[0] > 0, rz[1] > 0, qz[0] > 0, qz[1] > 0)
    hits, info = check(engine, tmp_path, refs, reads, sorted_=True)
    assert hits.sum() > 1000
    assert info["n_degenerate"] == nqi                                         # inverted queries are reported, and still matched


def test_a_zero_length_query_on_a_zero_length_region(engine, rng, tmp_path):
    """one zero-length query among ordinary ones, lying on a zero-length region: the two do not match (start <= stop fails either
    way), although the region ends before the query's start without starting at or before its stop -- the one pair a difference
    of ranks would get wrong.  The other queries' hits do not change"""
    refs, reads = regions(rng, 3000, 200_000, 1, 2000), regions(rng, 15_000, 200_000, 1, 200)
    refs["e"][100] = refs["s"][100] - 1; refs["blocks"][:, 1] = refs["e"]
    assert int((reads["s"] > reads["e"]).sum()) == 0
    plain, _ = check(engine, tmp_path, refs, reads, sorted_=True)
    x = np.array([refs["s"][100]])
    one = dict(chrom=np.array([refs["chrom"][100]]), strand=np.array([0]), s=x, e=x - 1, first=np.array([0, 1]), blocks=np.stack([x, x - 1], axis=1))
    reads = concat(reads, one)
    reads = take(reads, np.lexsort((reads["s"], reads["chrom"])))              # (stable: the others keep their order)
    z = np.flatnonzero(reads["s"] > reads["e"])
    assert len(z) == 1
    hits, info = check(engine, tmp_path, refs, reads, sorted_=True)
    assert np.array_equal(np.delete(hits, z[0]), plain) and info["n_degenerate"] == 0


def test_zero_length_queries_without_the_merge_are_degenerate(engine, rng, tmp_path):
    """the bin index's rule: start > stop is reported and has no hits (the reference exits, :5740-5741; the caller's business)"""
    refs, reads = regions(rng, 3000, 200_000, 1, 2000), regions(rng, 15_000, 200_000, 1, 200)
    want, tri, _, _ = setup(engine, tmp_path, refs, reads)
    tri[5000, 2] = tri[5000, 1] - 1
    tri[9000, 2] = tri[9000, 1] - 20
    hits, info = engine.query_hits(tri)
    off, _, jinfo = engine.join(tri, capacity=0)
    want[[5000, 9000]] = 0
    assert np.array_equal(hits, want) and np.array_equal(hits, np.diff(off)) and info == jinfo
    assert info["n_degenerate"] == 2 and info["first_degenerate"] == 5000


def test_query_hits_device(engine, rng, tmp_path):
    torch = pytest.importorskip("torch")
    refs, reads = regions(rng, **R), regions(rng, **Q)
    for kw in (dict(), dict(sorted_=True), dict(ign=False)):
        want, tri, _, flags = setup(engine, tmp_path, refs, reads, **kw)
        d_reads = torch.from_numpy(tri).cuda()
        d_hits = torch.full((len(tri),), 0x7fffffff, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        info = engine.query_hits_device(d_reads.data_ptr(), len(tri), d_hits.data_ptr(), flags)
        assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), want)
        assert info["n_no_class"] == 0 and info["n_degenerate"] == 0 and info["first_unsorted"] == -1
    # one inverted query under the merge
    want, tri, _, flags = setup(engine, tmp_path, refs, reads, sorted_=True)
    tri[777, 2] = tri[777, 1] - 30
    d_reads = torch.from_numpy(tri).cuda()
    d_hits = torch.full((len(tri),), 0x7fffffff, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    info = engine.query_hits_device(d_reads.data_ptr(), len(tri), d_hits.data_ptr(), flags)
    off, _, jinfo = engine.join(tri, flags, capacity=0)
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), np.diff(off)) and info == jinfo and info["n_degenerate"] == 1
    assert np.array_equal(np.delete(np.diff(off), 777), np.delete(want, 777))


def test_check_sorted_reports_the_first_violation_across_batches(engine, rng, tmp_path):
    """GTX_CHECK_SORTED as in gtx_join: a violation at the seam between two host batches comes before one inside the second
    batch; batches do not show in the hits"""
    refs, reads = regions(rng, 2000, 300_000, 1, 3000), regions(rng, 5000, 300_000, 1, 300)
    setup(engine, tmp_path, refs, reads, sorted_=True)
    t = triples(reads, True)
    hits_ok, info_ok = engine.query_hits(t, gtx.ZERO_LENGTH_OK | gtx.CHECK_SORTED)
    assert info_ok["first_unsorted"] == -1
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
        hits, info = e.query_hits(t, gtx.ZERO_LENGTH_OK | gtx.CHECK_SORTED)
        off, _, jinfo = e.join(t, gtx.ZERO_LENGTH_OK | gtx.CHECK_SORTED, capacity=0)
        assert info["first_unsorted"] == 3000 and info == jinfo and np.array_equal(hits, np.diff(off))
        hits_all, info_all = engine.query_hits(t, gtx.ZERO_LENGTH_OK | gtx.CHECK_SORTED)
        assert info_all["first_unsorted"] == 3000 and np.array_equal(hits, hits_all)
        t[4000] = triples(reads, True)[4000]; t[3000] = triples(reads, True)[3000]
        assert np.array_equal(e.query_hits(t, gtx.ZERO_LENGTH_OK)[0], hits_ok)
    finally:
        e.close()


def test_argument_and_call_order_errors(engine, rng):
    e = gtx.Engine(0)
    try:
        t = np.array([[0, 1, 10]], dtype=np.int32)
        out = np.zeros(1, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert e.lib.gtx_query_hits(e.ctx, p(t), None, None, 1, 0, p(out), None) == E_STATE
        assert b"gtx_set_refs has not been called" in e.lib.gtx_last_error(e.ctx)
        assert e.lib.gtx_query_hits_device(e.ctx, None, 0, 0, None, None) == E_STATE
        e.set_refs(np.array([[0, 5, 20]], dtype=np.int32), 1)
        assert e.lib.gtx_query_hits(e.ctx, p(t), None, None, -1, 0, p(out), None) == E_ARG
        assert e.lib.gtx_query_hits(e.ctx, None, None, None, 1, 0, p(out), None) == E_ARG
        assert e.lib.gtx_query_hits(e.ctx, p(t), None, None, 1, 0, None, None) == E_ARG
        first = np.array([1, 2], dtype=np.int64)                                # first[0] != 0
        assert e.lib.gtx_query_hits(e.ctx, p(t), p(first), p(t), 1, 0, p(out), None) == E_ARG
        assert e.lib.gtx_query_hits_device(e.ctx, None, 1, 0, None, None) == E_ARG
        assert e.lib.gtx_query_hits_device(e.ctx, None, -1, 0, None, None) == E_ARG
        assert e.lib.gtx_query_hits(None, p(t), None, None, 1, 0, p(out), None) == E_ARG
        assert e.lib.gtx_query_hits(e.ctx, None, None, None, 0, 0, None, None) == OK      # no queries: nothing to do
        assert e.lib.gtx_query_hits(e.ctx, p(t), None, None, 1, 0, p(out), None) == OK and out[0] == 1
    finally:
        e.close()
