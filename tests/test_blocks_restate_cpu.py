"""The restatement of genomic_blocks' six operations (tests/blocks_restate.py) against the hand-derived manifest
(tests/golden/blocks_manifest.json), its second renderer run_plain against run on seeded plain lines, and its notion of a plain
line against the generators of tests/blocks_cases.py."""
import json
import os
import random

import pytest

import blocks_cases as bc
import blocks_restate as br

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "blocks_manifest.json")))["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_manifest_output(case):
    text = bc.text_of(case["input"])
    assert br.run(br.norm_op(case["op"]), text) == (case["stdout"], case["stderr"], case["code"])


def test_the_manifest_covers_what_it_must():
    assert len(CASES) >= 40 and len({c["name"] for c in CASES}) == len(CASES)
    assert all(c["source"] for c in CASES)
    for kind in br.KINDS:
        cols = {len(l.split("\t")) for c in CASES if c["op"]["kind"] == kind for l in c["input"]}
        assert {3, 4, 5, 6, 8, 9, 12} <= cols, (kind, cols)
    sel = [c for c in CASES if c["op"]["kind"] == "select"]
    assert any(not any(c["op"].get(f) for f in br.SELECT_FLAGS) for c in sel)
    for f in br.SELECT_FLAGS:
        for strand in "+-":
            assert any(c["op"].get(f) and not any(c["op"].get(g) for g in br.SELECT_FLAGS if g != f) and ("\t%s\t" % strand) in c["input"][0] for c in sel), (f, strand)
    both = {int(c["input"][0].split("\t")[9]) for c in sel if c["op"].get("first") and c["op"].get("last")}
    assert {1, 2, 3, 5} <= both
    assert any(c["code"] == 1 and "sorted and non-overlapping" in c["stderr"] for c in CASES)
    assert any(c["code"] == 1 and "exons cannot overlap" in c["stderr"] and not c["stdout"].endswith("\n") for c in CASES)
    assert any(c["op"].get("op") not in (None, "+", "-", "r") for c in CASES)
    assert any(l.startswith("track ") for c in CASES for l in c["input"])


@pytest.mark.parametrize("op", bc.ops(), ids=bc.op_id)
def test_run_plain_equals_run_on_seeded_plain_lines(op):
    rng = random.Random(7)
    lines = [bc.plain(rng) for _ in range(2500)]
    assert sum(len(l.split("\t")) == 12 for l in lines) >= 1000 and sum(len(l.split("\t")) < 12 for l in lines) >= 500
    text = bc.text_of(lines)
    want = br.run(op, text)
    assert want[1:] == ("", 0)
    assert br.run_plain(op, text) == want[0]


def test_generated_plain_lines_are_plain_and_odd_lines_are_not():
    rng = random.Random(3)
    for _ in range(3000):
        assert br.is_plain(bc.plain(rng))
    for n in (1, 2, 63, 64, 65, br.MAX_BLOCKS - 1, br.MAX_BLOCKS):
        for comma in (False, True):
            assert br.is_plain(bc.plain12(rng, n, comma=comma, max_gap=50))
    assert not br.is_plain(bc.plain12(rng, br.MAX_BLOCKS + 1, max_gap=50))
    for kind in bc.ODD_KINDS:
        for _ in range(200):
            line = bc.odd(rng, kind)
            assert not br.is_plain(line), (kind, line)
    for line in ("chr1\t5", "chr1\t5\t9\t", "chr1\t5\t9\tx\t-0", "chr1\t2147483645\t2147483646", "chr1\t5\t2147483646",
                 "chr1\t100\t200\tu\t0\t+\t100\t200\t0\t2\t10,10\t50,0", "chr1\t100\t200\tv\t0\t+\t100\t200\t0\t2\t60,50\t0,50",
                 "chr1\t100\t200\tv\t0\t+\t100\t200\t0\t0\t\t", "chr1\t100\t200\tv\t0\t+\t100\t2147483646\t0\t1\t100\t0"):
        assert not br.is_plain(line), line
    assert br.is_plain("chr1\t2147483644\t2147483645") and br.is_plain("chr1\t0\t30\tx\t0\t+\t0\t30\t0\t3\t10,10,10\t0,10,20")


def test_every_odd_kind_runs_through_every_operation_without_an_error():
    rng = random.Random(5)
    text = bc.text_of([bc.odd(rng, k) for k in bc.ODD_KINDS for _ in range(20)])
    for op in bc.ops():
        assert br.run(op, text)[1:] == ("", 0), op
