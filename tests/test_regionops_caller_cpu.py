"""CPU suite: the host loop of GenomicRegionSet::RunShiftPos / RunModifyPos / RunCenter / RunFix / RunBounds (csrc/gtx_host_regionops.cpp),
called by tests/tools/regionops_caller.cpp the way genomic_regions calls them, against the restatement (tests/regionops_restate.py): the
manifest's cases, and a few hundred seeded lines per operation -- plain ones mixed with space-separated lines, '.', '1' and '-1'
strands, leading zeros and signs, 7 to 12 columns (BED12 with its blocks) -- ending in a 2-token line that must give the reference's
error behind the output in front of it.  No GPU is involved: the caller says GTX_TEXT_ON_DEVICE=0 and the loop looks for no device."""
import json
import os
import subprocess

import numpy as np
import pytest

import regionops_restate as rr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CALLER = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "regionops_caller")
CASES = json.load(open(os.path.join(HERE, "golden", "regionops_manifest.json")))["cases"]
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
GENOME = {"chr1": 200_000, "chr2": 150_000}                        # chr3 is absent; chr2's bound cuts into its lines


def caller_args(op):
    k = op["kind"]
    if k in ("shift", "shiftp"):
        return [k, str(op["a"]), str(op["b"])]
    if k == "pos":
        return [k, op["op"], str(op["c"])]
    if k == "bounds":
        return [k, "genome.bed"]
    return [k]


def caller(tmp, op, text):
    (tmp / "in.bed").write_text(text)
    if op["kind"] == "bounds":
        (tmp / "genome.bed").write_text("".join("%s\t0\t%d\n" % (c, n) for c, n in op["genome"].items()))
    r = subprocess.run([CALLER] + caller_args(op) + ["in.bed"], capture_output=True, cwd=tmp, env=ENV)
    return r.stdout.decode(), r.stderr.decode(), r.returncode


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_caller_gives_the_manifest_output(tmp_path, case):
    assert caller(tmp_path, case["op"], "".join(l + "\n" for l in case["input"])) == (case["stdout"], case["stderr"], case["code"])


def seeded_lines(seed, n=300):
    """mixed plain and odd lines on three chromosomes, a 2-token line last"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        c = "chr%d" % rng.integers(1, 4)
        s = int(rng.integers(0, 210_000)); ln = int(rng.integers(-40, 3000))
        cols = [c, str(s), str(s + ln), "r%d" % k, str(int(rng.integers(-5, 1000))), "+-"[int(rng.integers(0, 2))]]
        kind = int(rng.integers(0, 12))
        if kind < 5:
            line = "\t".join(cols[:int(rng.integers(3, 7))])                       # plain, 3 to 6 columns
        elif kind == 5:
            line = " ".join(cols[:int(rng.integers(3, 7))])                        # space-separated
        elif kind == 6:
            line = "\t".join(cols[:5] + [[".", "1", "-1"][int(rng.integers(0, 3))]])
        elif kind == 7:
            line = "\t".join([c, "00%d" % s, "+%d" % (s + ln), cols[3], "007"])    # leading zeros, a sign, a score that is not canonical
        elif kind == 8:
            line = "\t".join([c, "-%d" % (s % 50), str(ln + 40)] + cols[3:])       # a negative start column
        elif kind == 9:
            line = "\t".join(cols + [str(s + 5)])                                  # 7 columns: six are printed
        elif kind == 10:
            line = "\t".join(cols + [str(s + 5), str(s + 9), "255,0,0"][:int(rng.integers(2, 4))])   # 8 or 9 columns: thickStart / thickEnd
        else:                                                                     # BED12: sorted, disjoint blocks
            nb = int(rng.integers(1, 5)); sizes = [int(rng.integers(5, 60)) for _ in range(nb)]
            starts = [0]
            for z in sizes[:-1]:
                starts.append(starts[-1] + z + int(rng.integers(1, 80)))
            end = s + starts[-1] + sizes[-1]
            line = "\t".join([c, str(s), str(end), cols[3], cols[4], cols[5], str(s + 2), str(end - 1), "0", str(nb),
                              ",".join(map(str, sizes)) + ",", ",".join(map(str, starts)) + ","])
        out.append(line)
    out.append("chr1\t77")
    return "".join(l + "\n" for l in out)


OPS = [{"kind": "shift", "a": 150, "b": -90}, {"kind": "shift", "a": -3000, "b": 25}, {"kind": "shiftp", "a": -500, "b": 1200},
       {"kind": "pos", "op": "1", "c": 50}, {"kind": "pos", "op": "2", "c": 50}, {"kind": "pos", "op": "5p", "c": 0}, {"kind": "pos", "op": "3p", "c": 700},
       {"kind": "pos", "op": "c", "c": 20}, {"kind": "center"}, {"kind": "fix"}, {"kind": "bounds", "genome": GENOME}]


@pytest.mark.parametrize("op", OPS, ids=lambda o: "-".join(str(v) for v in o.values() if not isinstance(v, dict)))
def test_caller_equals_the_restatement_on_seeded_lines(tmp_path, op):
    text = seeded_lines(11 + OPS.index(op))
    want = rr.run(op, text)
    assert want[2] == 1 and want[1] == "\nError: Line 301: number of tokens should be at least 3 for BED format!\n"
    assert want[0].count("\n") > (100 if op["kind"] in ("fix", "bounds") else 290)
    assert sum(not rr.is_plain(l) for l in text.split("\n")[:-1]) > 100
    assert caller(tmp_path, op, text) == want
