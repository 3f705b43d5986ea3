"""CPU suite: the restatement of genomic_regions shift | shiftp | pos | center | fix | bounds (tests/regionops_restate.py) against the
hand-derived cases of tests/golden/regionops_manifest.json, and its two readings of a plain line -- the reader and Print, and
"copy columns 1 and 4-6, render 2 and 3" (what the device does) -- against each other."""
import json
import os

import pytest

import regionops_restate as rr

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "regionops_manifest.json")))["cases"]


def text_of(lines):
    return "".join(l + "\n" for l in lines)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_manifest_output(case):
    assert rr.run(case["op"], text_of(case["input"])) == (case["stdout"], case["stderr"], case["code"])
    assert len(case["derivation"]) > 20


def test_manifest_covers_what_it_must():
    kinds = {c["op"]["kind"] for c in CASES}
    assert kinds == set(rr.KINDS)
    assert {c["op"]["op"] for c in CASES if c["op"]["kind"] == "pos"} >= set(rr.POS_OPS)
    widths = {len(l.split("\t")) for c in CASES for l in c["input"]}
    assert widths >= {3, 4, 5, 6}
    outs = "".join(c["stdout"] for c in CASES)
    assert "\t0\t" in outs and "\t-1\t" in outs
    assert any(l.endswith("-") for c in CASES for l in c["input"]) and any(l.endswith("+") for c in CASES for l in c["input"])


@pytest.mark.parametrize("case", [c for c in CASES if c["code"] == 0 and all(rr.is_plain(l) for l in c["input"])],
                         ids=lambda c: c["name"])
def test_on_plain_lines_the_copy_is_the_print(case):
    assert rr.run_plain(case["op"], text_of(case["input"])) == case["stdout"]


def test_plain_line_predicate():
    ok = ["c\t0\t1", "c\t10\t5\tl", "c\t1\t2\tl\t-7", "c\t1\t2\tl\t0\t-", "c\t2147483644\t2147483645"]
    bad = ["c 0 1", "c\t01\t2", "c\t1\t2\tl\t07", "c\t1\t2\tl\t-0", "c\t1\t2\tl\t1\t.", "c\t1\t2\tl\t1\t+\t7", "c\t1", "c\t-1\t2", "c\t1\t2\r",
           "c\t1\t2\t", "c\t12345678901\t2", "c\t2147483645\t2147483646", "c\t1\t2\ta b", "c\t1\t2\tl\t1\t-1"]
    assert all(rr.is_plain(l) for l in ok)
    assert not any(rr.is_plain(l) for l in bad)


def test_truncating_division():
    assert [rr.tdiv(a, 2) for a in (-9, -10, -1, 0, 1, 9)] == [-4, -5, 0, 0, 0, 4]
