"""genomic_windows (csrc/genomic_windows.cpp) without a GPU: with
GTX_TEXT_ON_DEVICE=0 the tool runs its host loop, which looks for no device, and must print the manifest's bytes
(tests/golden/windows_manifest.json) and the restatement's (tests/windows_restate.py) on a few thousand seeded lines, from a file
and from stdin; usage, help and option errors with the reference's options (gtools/genomic_regions.cpp:647-651); -d below 1 refused up
front; `genomic_regions win` still refused; and a run without a GPU ending in the library's error with nothing on stdout."""
import json
import os
import subprocess

import pytest

import windows_restate as wr
from windows_cases import OPS, seeded_lines

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
TOOL = os.path.join(CSRC, "genomic_windows")
REGIONS = os.path.join(CSRC, "genomic_regions")
CASES = json.load(open(os.path.join(HERE, "golden", "windows_manifest.json")))["cases"]


def tool_args(op):
    return ["-s", str(op["size"]), "-d", str(op["step"])] + (["--small"] if op["small"] else [])


def tool(args, cwd, stdin=None, host_loop=True, exe=TOOL):
    assert os.path.exists(exe), "%s has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)" % os.path.basename(exe)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    env.pop("GTX_TEXT_ON_DEVICE", None)
    if host_loop:
        env["GTX_TEXT_ON_DEVICE"] = "0"
    r = subprocess.run([exe] + args, capture_output=True, cwd=cwd, env=env, input=stdin)
    return r.stdout.decode(), r.stderr.decode(), r.returncode


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_gives_the_manifest_output(tmp_path, case):
    text = "".join(l + "\n" for l in case["input"])
    (tmp_path / "in.bed").write_text(text)
    want = (case["stdout"], case["stderr"], case["code"])
    assert tool(tool_args(case["op"]) + ["in.bed"], tmp_path) == want
    assert tool(tool_args(case["op"]), tmp_path, stdin=text.encode()) == want


@pytest.mark.parametrize("op", OPS, ids=lambda o: "d%d-s%d-%s" % (o["step"], o["size"], "small" if o["small"] else "full"))
def test_host_loop_equals_the_restatement_on_seeded_lines(tmp_path, op):
    text = seeded_lines(3 + OPS.index(op))
    want = wr.run(op, text)
    assert want[2] == 1 and want[1] == "\nError: Line 3001: this operation requires single-interval regions!\n\n"
    assert sum(not wr.is_plain(l) for l in text.split("\n")[:-1]) > 1000
    (tmp_path / "in.bed").write_text(text)
    assert tool(tool_args(op) + ["in.bed"], tmp_path) == want
    assert tool(tool_args(op), tmp_path, stdin=text.encode()) == want


def test_help_and_option_errors(tmp_path):
    out, err, rc = tool(["-h"], tmp_path)
    assert rc == 1 and out == ""
    assert "genomic_windows [OPTIONS] <REGION-SET>" in err
    for o, text in [("--help", "help"), ("-h", "help"), ("-v", "verbose mode"), ("-s", "window size"), ("-d", "window distance"),
                    ("--small", "include smaller windows at the end of chromosomes")]:
        assert "\n  %-25s %s\n" % (o, text) in err, o
    assert "Creates new invervals by sliding windows." in err and "Input formats: BED" in err and "Region requirements: single-interval" in err
    assert "--ngpu" not in err
    assert tool(["--help"], tmp_path) == (out, err, rc)
    assert tool(["--bogus", "a.bed"], tmp_path) == ("", "Error: unknown option '--bogus'!\n", 1)
    assert tool(["--ngpu", "2", "a.bed"], tmp_path) == ("", "Error: unknown option '--ngpu'!\n", 1)
    assert tool(["-s"], tmp_path) == ("", "Error: could not set option '-s'!\n", 1)
    assert tool(["-d"], tmp_path) == ("", "Error: could not set option '-d'!\n", 1)


def test_a_distance_below_one_is_refused_up_front(tmp_path):
    (tmp_path / "a.bed").write_text("track name=x\nchr1\t0\t10\n")
    for d in ("0", "-4"):
        for host_loop in (True, False):
            assert tool(["-d", d, "a.bed"], tmp_path, host_loop=host_loop) == ("", "Error: window distance must be at least 1!\n", 1)


def test_genomic_regions_still_refuses_win(tmp_path):
    out, err, rc = tool(["win", "-s", "5", "a.bed"], tmp_path, exe=REGIONS)
    assert (out, rc) == ("", 1) and err == "Operation 'win' is outside the MI355X path of this build!\n"


def test_a_set_that_is_not_bed_is_unsupported(tmp_path):
    (tmp_path / "a.sam").write_text("@HD\tVN:1.0\nr1\t0\tchr1\t5\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n")
    (tmp_path / "a.gff").write_text("chr1\tsrc\tgene\t5\t30\t.\t+\t.\tID=g\n")
    for name in ("a.sam", "a.gff"):
        out, err, rc = tool([name], tmp_path)
        assert rc == 1 and out == "" and "unsupported input format!" in err


def test_an_empty_set_prints_nothing(tmp_path):
    (tmp_path / "a.bed").write_text("")
    assert tool(["a.bed"], tmp_path) == ("", "", 0)


def test_without_a_gpu_the_run_fails_with_the_librarys_error(tmp_path):
    """whatever the input's size the device is looked for: a run may not quietly take the host loop"""
    (tmp_path / "a.bed").write_text("chr1\t0\t10\ta\n")
    for args, stdin in ((["-s", "5", "a.bed"], None), (["-s", "5"], b"chr1\t0\t10\n"), (["-s", "0", "a.bed"], None)):
        out, err, rc = tool(args, tmp_path, stdin, host_loop=False)
        assert rc == 1 and out == ""
        assert "no usable HIP device" in err and "no CPU path" in err
