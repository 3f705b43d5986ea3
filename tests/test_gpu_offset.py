"""Pair offsets (gtx_join_offsets / gtx_pair_offsets_device, include/gtx.h; kernels in csrc/gtx_offset.hip).  Expected values:
the oracle's `pairs` rows (oracle/gtx_oracle.c: the (query, index region) pairs in the reference's iteration order) restated
through GenomicInterval::GetOffsetFrom (genomic_intervals.cpp:646-667) and CalcOffsetsWithoutGaps (:6154-6205) in
oracle/restate.py.  Without -S the index is the reference set and the point is the reference region; under -S (the oracle run
as `pairs -S test.bed refs.bed`) the merge's queries are the reference regions and the point is the query."""
import functools
import subprocess

import numpy as np
import pytest

import gtx
from oracle import orc, restate
from oracle.restate import NAMES, bin_keys, concat, multi, offset_from, offsets_without_gaps, take, triples, write_bed

pytestmark = pytest.mark.gpu

OPS = ["1", "2", "5p", "3p"]
regions = functools.partial(restate.regions, block_max=400)


def inside(rng, refs, n):
    """n queries whose intervals lie inside the intervals of random multi-interval reference regions (the skip-gaps entries)"""
    cand = np.flatnonzero(np.diff(refs["first"]) > 1)
    first, blocks, chrom, strand, s, e = [0], [], [], [], [], []
    for k in rng.choice(cand, n):
        iv = []
        for a, b in refs["blocks"][refs["first"][k]:refs["first"][k + 1]]:
            if rng.random() < 0.7:
                x = int(rng.integers(a, b + 1)); y = int(rng.integers(x, b + 1)); iv.append((x, y))
        if not iv:
            a, b = refs["blocks"][refs["first"][k]]; iv = [(int(a), int(b))]
        blocks += iv; first.append(len(blocks))
        chrom.append(refs["chrom"][k]); strand.append(refs["strand"][k]); s.append(iv[0][0]); e.append(iv[-1][1])
    r = dict(chrom=np.array(chrom), strand=np.array(strand), s=np.array(s, dtype=np.int64), e=np.array(e, dtype=np.int64),
             first=np.array(first, dtype=np.int64), blocks=np.array(blocks, dtype=np.int64).reshape(-1, 2))
    return take(r, np.lexsort((r["s"], r["chrom"])))


def intervals(r, i):
    return [(int(a), int(b)) for a, b in r["blocks"][r["first"][i]:r["first"][i + 1]]]


def oracle_rows(tmp, args, index, queries):
    r = subprocess.run([orc.CLI, "pairs"] + args + [index, queries], capture_output=True, cwd=tmp)
    assert r.returncode == 0, r.stderr.decode()
    return [(int(a) - 1, int(b[1:])) for a, b in (x.split("\t") for x in r.stdout.decode().splitlines())]


def expected(rows, refs, tests, op, sorted_, skip):
    """per row the entries: without -S rows are (test, ref), under -S (ref, test)"""
    out = []
    for a, b in rows:
        if sorted_:
            k, t = a, b
            out.append([offset_from(intervals(refs, k), refs["strand"][k] == 1, op, int(tests["s"][t]), int(tests["e"][t]))])
        else:
            t, k = a, b
            riv, minus = intervals(refs, k), refs["strand"][k] == 1
            out.append(offsets_without_gaps(intervals(tests, t), riv, minus, op) if skip else
                       [offset_from(riv, minus, op, int(tests["s"][t]), int(tests["e"][t]))])
    return out


def run(engine, tmp, refs, tests, op, sorted_=False, ign=True, gaps=False, skip=False, buffer=None):
    """(oracle rows, expected entries per row, the engine's offsets / pairs / entry offsets / entries / first inverted)"""
    write_bed(tmp / "refs.bed", refs, "r")
    write_bed(tmp / "tests.bed", tests, "q")
    args = (["-S"] if sorted_ else []) + (["-i"] if ign else []) + (["-gaps"] if gaps else [])
    rows = oracle_rows(tmp, args, "tests.bed", "refs.bed") if sorted_ else oracle_rows(tmp, args, "refs.bed", "tests.bed")
    index, queries = (tests, refs) if sorted_ else (refs, tests)
    n_classes = len(NAMES) * (1 if ign else 2)
    engine.set_refs(triples(index, ign), n_classes, gtx.REFS_KEEP_ZERO_LENGTH if sorted_ else 0)
    mi = multi(index)
    engine.set_ref_blocks(*mi) if mi else engine.set_ref_blocks(None)
    engine.set_ref_order(None if sorted_ else bin_keys(index))
    engine.set_ref_strands(index["strand"])
    engine.set_join_buffer(buffer or (1 << 26))
    flags = (gtx.ZERO_LENGTH_OK | gtx.OFFSET_FROM_QUERY if sorted_ else 0) | (gtx.JOIN_GAPS if gaps else 0) | (gtx.OFFSET_SKIP_REF_GAPS if skip else 0)
    mq = multi(queries)
    got = engine.join_offsets(triples(queries, ign), op, flags, *(mq or (None, None)), strands=queries["strand"] if sorted_ else None)
    return rows, expected(rows, refs, tests, op, sorted_, skip), got


def got_rows(off, pairs):
    return [(i, int(k)) for i in range(len(off) - 1) for k in pairs[off[i]:off[i + 1]]]


def got_entries(eoff, ent):
    return [[tuple(int(v) for v in ent[e]) for e in range(eoff[p], eoff[p + 1])] for p in range(len(eoff) - 1)]


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(4242)


@pytest.mark.parametrize("sorted_", [False, True], ids=["bin", "merge"])
@pytest.mark.parametrize("ign", [True, False], ids=["i", "strand"])
@pytest.mark.parametrize("op", OPS)
def test_offsets_equal_the_restated_reference(engine, rng, tmp_path, op, ign, sorted_):
    refs = regions(rng, 2000, 300_000, 1, 4000, multi=0.3)
    tests = regions(rng, 12_000, 300_000, 1, 300)
    rows, want, (off, pairs, eoff, ent, inv, info) = run(engine, tmp_path, refs, tests, op, sorted_=sorted_, ign=ign)
    assert len(rows) > 1000 and set(refs["strand"]) == {0, 1}
    assert got_rows(off, pairs) == rows
    assert np.array_equal(eoff, np.arange(len(rows) + 1))
    assert got_entries(eoff, ent) == want
    assert inv == -1 and info["n_no_class"] == 0


@pytest.mark.parametrize("sorted_", [False, True], ids=["bin", "merge"])
def test_bed12_on_both_sides_and_gaps(engine, rng, tmp_path, sorted_):
    """BED12 reference regions (the point's front / back interval) and, under -S, BED12 queries (the reference file); -gaps: the
    envelopes decide the pairs"""
    refs = regions(rng, 2000, 300_000, 1, 3000, multi=0.6)
    tests = regions(rng, 10_000, 300_000, 1, 300)
    for gaps in (False, True):
        rows, want, (off, pairs, eoff, ent, _, _) = run(engine, tmp_path, refs, tests, "3p", sorted_=sorted_, gaps=gaps)
        assert len(rows) > 1000 and got_rows(off, pairs) == rows and got_entries(eoff, ent) == want


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("ign", [True, False], ids=["i", "strand"])
def test_skip_ref_gaps(engine, rng, tmp_path, op, ign):
    refs = regions(rng, 1500, 300_000, 1, 3000, multi=0.6)
    tests = concat(regions(rng, 6000, 300_000, 1, 200, multi=0.3), inside(rng, refs, 3000))
    tests = take(tests, np.lexsort((tests["s"], tests["chrom"])))
    rows, want, (off, pairs, eoff, ent, inv, _) = run(engine, tmp_path, refs, tests, op, ign=ign, skip=True)
    assert got_rows(off, pairs) == rows
    assert got_entries(eoff, ent) == want
    assert sum(len(w) > 1 for w in want) > 300 and sum(len(w) == 0 for w in want) > 300    # several entries; none
    assert inv == -1


def test_skip_ref_gaps_in_chunks(engine, rng, tmp_path):
    """a join buffer of 500 pairs: the entry offsets run on across chunks"""
    refs = regions(rng, 1500, 300_000, 1, 3000, multi=0.6)
    tests = concat(regions(rng, 6000, 300_000, 1, 200, multi=0.3), inside(rng, refs, 3000))
    tests = take(tests, np.lexsort((tests["s"], tests["chrom"])))
    rows, want, (off, pairs, eoff, ent, _, _) = run(engine, tmp_path, refs, tests, "5p", skip=True, buffer=500)
    assert len(rows) > 5000 and got_rows(off, pairs) == rows and got_entries(eoff, ent) == want


@pytest.mark.parametrize("sorted_", [False, True], ids=["bin", "merge"])
def test_chunks(engine, rng, tmp_path, sorted_):
    refs = regions(rng, 2000, 300_000, 1, 4000)
    tests = regions(rng, 12_000, 300_000, 1, 3000)
    rows, want, (off, pairs, eoff, ent, _, _) = run(engine, tmp_path, refs, tests, "5p", sorted_=sorted_, buffer=777)
    assert len(rows) > 5000 and got_rows(off, pairs) == rows and got_entries(eoff, ent) == want


def test_zero_length_and_inverted_under_the_merge(engine, rng, tmp_path):
    """-S: zero-length and inverted regions pair by the merge's two comparisons; an inverted (or zero-length) test region gives a
    start offset above its stop offset, and the first such pair is reported"""
    refs = regions(rng, 2000, 200_000, 1, 3000)
    tests = regions(rng, 10_000, 200_000, 1, 200)
    for r in (refs, tests):
        n = len(r["s"])
        z = rng.random(n) < 0.05
        r["e"][z] = r["s"][z] - 1
        inv = (rng.random(n) < 0.05) & ~z
        r["e"][inv] = r["s"][inv] - rng.integers(2, 50, size=int(inv.sum()))
        r["blocks"][:, 1] = r["e"]
    rows, want, (off, pairs, eoff, ent, inv, _) = run(engine, tmp_path, refs, tests, "5p", sorted_=True)
    assert len(rows) > 1000 and got_rows(off, pairs) == rows and got_entries(eoff, ent) == want
    bad = [p for p, w in enumerate(want) if w[0][0] > w[0][1]]
    assert bad and inv == bad[0]


def test_unknown_chromosomes_pair_with_nothing(engine, rng, tmp_path):
    refs = regions(rng, 2000, 300_000, 1, 3000, n_chrom=2)
    tests = regions(rng, 10_000, 300_000, 1, 300, n_chrom=3)
    for sorted_ in (False, True):
        rows, want, (off, pairs, eoff, ent, _, _) = run(engine, tmp_path, refs, tests, "5p", sorted_=sorted_)
        assert len(rows) > 500 and got_rows(off, pairs) == rows and got_entries(eoff, ent) == want
    off_u = engine.join_offsets(triples(tests, True, n_known=2), "5p")[0]
    assert np.diff(off_u)[tests["chrom"] == 2].sum() == 0 and (tests["chrom"] == 2).sum() > 0


def test_bad_arguments_are_errors(engine, rng):
    refs = regions(rng, 100, 10_000, 1, 300)
    engine.set_refs(triples(refs, True), len(NAMES))
    for op in (0, 5):
        with pytest.raises(gtx.GtxError):
            engine.join_offsets(triples(refs, True), op)
    with pytest.raises(gtx.GtxError):
        engine.join_offsets(triples(refs, True), "5p", gtx.OFFSET_SKIP_REF_GAPS | gtx.OFFSET_FROM_QUERY)


@pytest.mark.parametrize("op", OPS)
def test_pair_offsets_device_equals_the_host_path(engine, rng, tmp_path, op):
    torch = pytest.importorskip("torch")
    refs = regions(rng, 3000, 400_000, 1, 4000, multi=0.3)
    tests = regions(rng, 20_000, 400_000, 1, 3000)
    tests["s"][:5] = 100; tests["e"][:5] = 399_000                              # long segments: the block-per-query path
    tests["chrom"][:5] = 0; tests["blocks"][:5] = np.stack([tests["s"][:5], tests["e"][:5]], axis=1)
    tests = take(tests, np.lexsort((tests["s"], tests["chrom"])))
    rows, want, (off, pairs, eoff, ent, _, _) = run(engine, tmp_path, refs, tests, op)
    assert np.diff(off).max() > 500 and got_entries(eoff, ent) == want
    d_reads = torch.from_numpy(triples(tests, True)).cuda()
    d_off = torch.zeros(len(off), dtype=torch.int64, device="cuda")
    d_pairs = torch.zeros(int(off[-1]), dtype=torch.int32, device="cuda")
    total, done, _ = engine.join_device(d_reads.data_ptr(), len(off) - 1, d_off.data_ptr(), d_pairs.data_ptr(), int(off[-1]))
    assert total == off[-1] and done == len(off) - 1
    d_out = torch.full((int(total), 2), -7, dtype=torch.int64, device="cuda")
    inv = engine.pair_offsets_device(d_reads.data_ptr(), done, d_off.data_ptr(), d_pairs.data_ptr(), total, d_out.data_ptr(), op)
    assert inv == -1
    assert np.array_equal(d_out.cpu().numpy(), ent)
