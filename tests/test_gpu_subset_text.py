"""gtx_subset_text / gtx_subset_result through the C ABI (include/gtx.h; kernels in csrc/gtx_text.hip and csrc/gtx_query.hip): a
block of BED text in, the selected lines out byte for byte.  Expected: the lines whose count in the oracle's `qstats` is > 0
(== 0 under GTX_SUBSET_INVERT) on the same text; a block with a line that GenomicRegionBED::Print would not render as it stands
comes back whole."""
import ctypes
import subprocess

import numpy as np
import pytest

import gtx
from oracle import orc
from oracle.restate import NAMES, regions, triples, write_bed

pytestmark = pytest.mark.gpu


def oracle_counts(tmp, args, text):
    (tmp / "reads.bed").write_bytes(text)
    r = subprocess.run([orc.CLI, "qstats"] + args + ["refs.bed", "reads.bed"], capture_output=True, cwd=tmp)
    assert r.returncode == 0, r.stderr.decode()
    return np.array([int(x.split("\t")[1]) for x in r.stdout.decode().splitlines()])


def bed_text(r, cols=6):
    out = []
    for i in range(len(r["s"])):
        c = [NAMES[r["chrom"][i]], str(r["s"][i] - 1), str(r["e"][i]), "q%d" % i, str((-1) ** i * (i % 1000)), "+-"[r["strand"][i]]]
        out.append("\t".join(c[:cols]) + "\n")
    return out


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(31)


@pytest.mark.parametrize("sorted_,ign", [(False, True), (False, False), (True, True), (True, False)], ids=["bin -i", "bin", "merge -i", "merge"])
def test_blocks_of_text_select_what_the_oracle_counts(engine, rng, tmp_path, sorted_, ign):
    refs, reads = regions(rng, 1500, 400_000, 1, 400), regions(rng, 30_000, 400_000, 1, 400)
    write_bed(tmp_path / "refs.bed", refs, "r")
    # classes as the tokenizer numbers them: chromosome rank, + the number of chromosomes on the '-' strand
    t = triples(refs, True)
    if not ign:
        t[:, 0] += len(NAMES) * refs["strand"].astype(np.int32)
    engine.set_refs(t, len(NAMES) * (1 if ign else 2), gtx.REFS_KEEP_ZERO_LENGTH if sorted_ else 0)
    engine.set_ref_blocks(None)
    lines = bed_text(reads)
    cut = [0, 1, 9000, 9001, 22_000, len(lines)]                               # blocks of several sizes, one of a single line
    blocks = ["".join(lines[a:b]).encode() for a, b in zip(cut, cut[1:])]
    want = oracle_counts(tmp_path, (["-S"] if sorted_ else []) + (["-i"] if ign else []), b"".join(blocks))
    assert 0.1 < (want > 0).mean() < 0.9
    rules = gtx.TextRules.make(NAMES, strand_aware=not ign, sorted_rules=sorted_)
    flags = gtx.ZERO_LENGTH_OK if sorted_ else 0
    for inv in (0, gtx.SUBSET_INVERT):
        got = engine.subset_text(blocks, rules, flags | inv)
        assert [g[0] for g in got] == [0] * len(blocks)
        keep = (want == 0) if inv else (want > 0)
        assert b"".join(g[1] for g in got) == "".join(l for l, k in zip(lines, keep) if k).encode()
        assert [g[2] for g in got] == [int(keep[a:b].sum()) for a, b in zip(cut, cut[1:])]


ODD = ["chr1 100 200 q 0 +\n", "chr1\t0100\t200\n", "chr1\t+100\t200\tq\n", "chr1\t100\t200\tq\t0\t.\n", "chr1\t100\t200\tq\t0\t1\n", "chr1\t100\t200\tq\t1.5\t+\n",
       "chr1\t100\t200\tq\t007\t+\n", "chr1\t100\t200\tq\t-0\t+\n", "chr1\t100\t200\tq\t0\t+\t0\n", "chr1\t100\t200\r\n", "chr1\t100\t200\t\t0\t+\n",
       "chr1\t100\t200\tq r\t0\t+\n", "chr1\t100\t200\tq\t1234567890123456789\t+\n", "chr1\t100\t400\tq\t7\t+\t100\t400\t0\t2\t50,100,\t0,200,\n"]
FINE = ["chr1\t100\t200\n", "chr1\t0\t200\tq\n", "chr1\t100\t200\tq\t-7\t-\n", "chr1\t100\t200\tq\t123456789012345678\t+\n", "chrUn\t100\t200\tq\t0\t+\n"]


def test_only_lines_that_print_as_they_stand_are_copied(engine, rng, tmp_path):
    engine.set_refs(np.array([[0, 150, 160]], dtype=np.int32), len(NAMES))
    engine.set_ref_blocks(None)
    rules = gtx.TextRules.make(NAMES)
    pad = "".join("chr1\t%d\t%d\tp%d\t0\t+\n" % (10 * i, 10 * i + 5, i) for i in range(300))
    for line in FINE:
        (redo, out, n), = engine.subset_text([(pad + line).encode()], rules, 0)
        assert (redo, n) == (0, 2 if line.startswith("chr1") else 1), line    # p15 = [151, 155] overlaps, and the line does on chr1
        assert out == ("chr1\t150\t155\tp15\t0\t+\n" + (line if line.startswith("chr1") else "")).encode()
    for line in ODD:
        for text in (pad + line, line + pad, line):
            (redo, out, n), = engine.subset_text([text.encode()], rules, 0)
            assert redo != 0 and (out, n) == (b"", 0), line


def test_zero_length_and_inverted_queries_are_selected_by_the_merges_rules(engine, tmp_path):
    """under GTX_ZERO_LENGTH_OK a zero-length or inverted query matches by the merge's two comparisons; such lines print as they
    stand, so their block is selected on the device like any other: held to gtx_query_hits on the same triples (which
    tests/test_gpu_query_hits.py holds to the oracle)"""
    rules = gtx.TextRules.make(NAMES, sorted_rules=True)
    text = b"chr1\t100\t200\ta\t0\t+\nchr1\t150\t150\tz\t0\t+\nchr1\t160\t140\ti\t0\t+\nchr1\t300\t400\tb\t0\t+\n"
    tri = np.array([[0, 101, 200], [0, 151, 150], [0, 161, 140], [0, 301, 400]], dtype=np.int32)
    for refs in ([[0, 120, 170]], [[0, 120, 170], [0, 500, 450]], [[0, 151, 150], [0, 320, 330]]):
        engine.set_refs(np.array(refs, dtype=np.int32), len(NAMES), gtx.REFS_KEEP_ZERO_LENGTH)
        engine.set_ref_blocks(None)
        hits, _ = engine.query_hits(tri, gtx.ZERO_LENGTH_OK)
        assert hits[0] + hits[3] > 0
        for inv in (0, gtx.SUBSET_INVERT):
            redo, out, n = engine.subset_text([text], rules, gtx.ZERO_LENGTH_OK | inv)[0]
            keep = (hits == 0) if inv else (hits > 0)
            assert redo == 0 and n == int(keep.sum()) and out == b"".join(l for l, k in zip(text.splitlines(True), keep) if k)


def test_argument_and_call_order_errors(engine):
    e = gtx.Engine(0)
    try:
        rules = gtx.TextRules.make(NAMES)
        t = ctypes.c_int(-1)
        text = b"chr1\t1\t2\n"
        assert e.lib.gtx_subset_text(e.ctx, text, len(text), 1, ctypes.byref(rules), 0, ctypes.byref(t)) == -3      # no reference set
        e.set_refs(np.array([[0, 1, 5]], dtype=np.int32), len(NAMES))
        assert e.lib.gtx_subset_text(e.ctx, None, 0, 0, ctypes.byref(rules), 0, ctypes.byref(t)) == -1
        assert e.lib.gtx_subset_text(e.ctx, text, len(text), 1, None, 0, ctypes.byref(t)) == -1
        assert e.lib.gtx_subset_text(e.ctx, text, len(text), 1, ctypes.byref(rules), gtx.TEXT_SAM, ctypes.byref(t)) == -1
        redo, nb = ctypes.c_int(0), ctypes.c_size_t(0)
        out = ctypes.create_string_buffer(64)
        assert e.lib.gtx_subset_result(e.ctx, 0, ctypes.byref(redo), out, ctypes.byref(nb), None) == -3              # no such block
        for _ in range(2):
            assert e.lib.gtx_subset_text(e.ctx, text, len(text), 1, ctypes.byref(rules), 0, ctypes.byref(t)) == 0
        assert e.lib.gtx_subset_text(e.ctx, text, len(text), 1, ctypes.byref(rules), 0, ctypes.byref(t)) == -3      # a result has not been fetched
        for k in (0, 1):
            assert e.lib.gtx_subset_result(e.ctx, k, ctypes.byref(redo), out, ctypes.byref(nb), None) == 0
            assert (redo.value, out.raw[:nb.value]) == (0, text)
        assert e.lib.gtx_subset_result(e.ctx, 0, ctypes.byref(redo), out, ctypes.byref(nb), None) == -3              # ... only once
        assert e.lib.gtx_subset_result(e.ctx, 2, ctypes.byref(redo), out, ctypes.byref(nb), None) == -1
    finally:
        e.close()
