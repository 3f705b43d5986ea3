"""genomic_blocks (csrc/genomic_blocks.cpp) without a GPU: with GTX_TEXT_ON_DEVICE=0 the tool runs its host loop, which looks for no
device, and must print the manifest's bytes (tests/golden/blocks_manifest.json) and the restatement's (tests/blocks_restate.py) on
thousands of seeded lines per operation, from a file and from stdin; usage, help and option errors with the reference's option texts
(gtools/genomic_regions.cpp:600-605, :617-623); the six words still refused by genomic_regions; an empty set; and a run without a GPU
ending in the library's error with nothing on stdout."""
import json
import os
import subprocess

import pytest

import blocks_cases as bc
import blocks_restate as br

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
TOOL = os.path.join(CSRC, "genomic_blocks")
REGIONS = os.path.join(CSRC, "genomic_regions")
CASES = json.load(open(os.path.join(HERE, "golden", "blocks_manifest.json")))["cases"]


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
    text = bc.text_of(case["input"])
    (tmp_path / "in.bed").write_text(text)
    want = (case["stdout"], case["stderr"], case["code"])
    args = br.tool_args(br.norm_op(case["op"]))
    assert tool(args + ["in.bed"], tmp_path) == want
    assert tool(args, tmp_path, stdin=text.encode()) == want


@pytest.mark.parametrize("op", bc.ops(), ids=bc.op_id)
def test_host_loop_equals_the_restatement_on_seeded_lines(tmp_path, op):
    lines = bc.mixed(23 + bc.ops().index(op), 9000, odd_every=4)
    text = bc.text_of(lines)
    want = br.run(op, text)
    assert want[1:] == ("", 0) and want[0].count("\n") >= 3000
    assert sum(not br.is_plain(l) for l in lines) >= 1000
    (tmp_path / "in.bed").write_bytes(text.encode())
    assert tool(br.tool_args(op) + ["in.bed"], tmp_path) == want
    assert tool(br.tool_args(op), tmp_path, stdin=text.encode()) == want


def test_usage_help_and_option_errors(tmp_path):
    out, err, rc = tool([], tmp_path)
    assert (out, rc) == ("", 1) and "genomic_blocks OPERATION [OPTIONS] <REGION-SET>" in err
    for line in ("  connect    Connects intervals from minimum start to maximum stop position.\n",
                 "  diff       Computes the difference between successive intervals.\n",
                 "  n          Computes sum of lengths of intervals in a region (including possible overlaps).\n",
                 "  select     Selects a subset of intervals according to their position in the region.\n",
                 "  split      Splits regions into their intervals which are printed on separate lines.\n",
                 "  strand     Modifies interval strand information.\n"):
        assert line in err
    assert tool(["union", "a.bed"], tmp_path) == ("", "Unknown operation 'union'!\n", 1)
    out, err, rc = tool(["select", "-h"], tmp_path)
    assert (out, rc) == ("", 1) and "genomic_blocks select [OPTIONS] <REGION-SET>" in err
    for o, text in [("--help", "help"), ("-h", "help"), ("-v", "verbose mode"), ("-first", "select the first interval"), ("-last", "select the last interval"),
                    ("-5p", "select the first from the 5' end"), ("-3p", "select the first from the 3' end")]:
        assert "\n  %-25s %s\n" % (o, text) in err, o
    assert "Selects a subset of intervals according to their position in the region." in err and "Region requirements: chromosome/strand-compatible" in err
    assert "--ngpu" not in err
    assert tool(["select", "--help"], tmp_path) == (out, err, rc)
    out, err, rc = tool(["split", "--help"], tmp_path)
    assert (out, rc) == ("", 1) and "\n  %-25s %s\n" % ("--by-chrstrand", "sort and split by chromosome and strand (REG format only)") in err
    out, err, rc = tool(["strand", "--help"], tmp_path)
    assert (out, rc) == ("", 1) and "\n  %-25s %s\n" % ("-op", "strand operation (+=positive, -=negative, r=reverse)") in err
    assert "\n  -s " not in err and "Modifies interval strand information." in err
    for word, about in (("connect", "Connects intervals from minimum start to maximum stop position."), ("diff", "Computes the difference between successive intervals."),
                        ("n", "Computes sum of lengths of intervals in a region (including possible overlaps).")):
        out, err, rc = tool([word, "-h"], tmp_path)
        assert (out, rc) == ("", 1) and about in err and "-first" not in err
    assert tool(["strand", "-s", "a.bed"], tmp_path) == ("", "Error: unknown option '-s'!\n", 1)
    assert tool(["diff", "-first", "a.bed"], tmp_path) == ("", "Error: unknown option '-first'!\n", 1)
    assert tool(["split", "--ngpu", "2", "a.bed"], tmp_path) == ("", "Error: unknown option '--ngpu'!\n", 1)
    assert tool(["strand", "-op"], tmp_path) == ("", "Error: could not set option '-op'!\n", 1)


def test_an_input_error_ends_the_run_behind_the_lines_in_front(tmp_path):
    text = "chr1\t5\t9\tq\nchr1\t7\n"
    want = ("q\t4\n", "\nError: Line 2: number of tokens should be at least 3 for BED format!\n", 1)
    assert br.run(br.make_op("n"), text) == want
    assert tool(["n"], tmp_path, stdin=text.encode()) == want


def test_an_empty_set_prints_nothing(tmp_path):
    (tmp_path / "a.bed").write_text("")
    for word in br.KINDS:
        assert tool([word, "a.bed"], tmp_path) == ("", "", 0)
        assert tool([word], tmp_path, stdin=b"") == ("", "", 0)


def test_without_a_gpu_the_run_fails_with_the_librarys_error(tmp_path):
    """whatever the input's size the device is looked for: a run may not quietly take the host loop"""
    (tmp_path / "a.bed").write_text("chr1\t100\t200\tT1\t5\t-\t120\t180\t0\t3\t10,20,30,\t0,40,70,\n")
    for args, stdin in ((["split", "a.bed"], None), (["n"], b"chr1\t0\t10\n"), (["strand", "-op", "x", "a.bed"], None), (["select", "-first", "a.bed"], None)):
        out, err, rc = tool(args, tmp_path, stdin, host_loop=False)
        assert rc == 1 and out == ""
        assert "no usable HIP device" in err and "no CPU path" in err


def test_genomic_regions_still_refuses_the_six_words(tmp_path):
    for word in br.KINDS:
        out, err, rc = tool([word, "a.bed"], tmp_path, exe=REGIONS)
        assert (out, rc) == ("", 1) and err == "Operation '%s' is outside the MI355X path of this build!\n" % word
