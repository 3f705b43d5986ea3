"""CPU suite: the host loop of GenomicRegionSet::RunSlidingWindows (csrc/gtx_host_regionops.cpp), called by
tests/tools/windows_caller.cpp the way genomic_regions calls it, against the manifest (tests/golden/windows_manifest.json) and, on
a few thousand seeded lines per set of options, the restatement (tests/windows_restate.py).  No GPU is involved: the caller says
GTX_TEXT_ON_DEVICE=0 and the loop looks for no device."""
import json
import os
import subprocess

import pytest

import windows_restate as wr
from windows_cases import OPS, seeded_lines

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CALLER = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "windows_caller")
CASES = json.load(open(os.path.join(HERE, "golden", "windows_manifest.json")))["cases"]
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


def caller(tmp, op, text):
    assert os.path.exists(CALLER), "windows_caller has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)"
    (tmp / "in.bed").write_text(text)
    r = subprocess.run([CALLER, str(op["step"]), str(op["size"]), "1" if op["small"] else "0", "in.bed"], capture_output=True, cwd=tmp, env=ENV)
    return r.stdout.decode(), r.stderr.decode(), r.returncode


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_caller_gives_the_manifest_output(tmp_path, case):
    assert caller(tmp_path, case["op"], "".join(l + "\n" for l in case["input"])) == (case["stdout"], case["stderr"], case["code"])


@pytest.mark.parametrize("op", OPS, ids=lambda o: "d%d-s%d-%s" % (o["step"], o["size"], "small" if o["small"] else "full"))
def test_caller_equals_the_restatement_on_seeded_lines(tmp_path, op):
    text = seeded_lines(40 + OPS.index(op))
    want = wr.run(op, text)
    assert want[2] == 1 and "Line 3001" in want[1]
    assert caller(tmp_path, op, text) == want


def test_the_class_api_refuses_a_distance_below_one(tmp_path):
    """behind the header the open set has echoed"""
    assert caller(tmp_path, {"step": 0, "size": 1, "small": False}, "track name=x\nchr1\t0\t10\n") == \
        ("track name=x\n", "Error: window distance must be at least 1!\n", 1)
