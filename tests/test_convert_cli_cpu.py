"""genomic_convert (csrc/genomic_convert.cpp) without a GPU: with GTX_TEXT_ON_DEVICE=0 the tool runs its host loop, which looks for
no device, and must print the manifest's bytes (tests/golden/convert_manifest.json) and the restatement's (tests/convert_restate.py)
on a few thousand seeded lines per format, from a file and from stdin; usage, help and option errors with the reference's options
(gtools/genomic_regions.cpp:485-490, :583-585); `bed` on a BED set refused; an input error behind the lines in front of it;
`genomic_regions bed` and `reg` still refused; and a run without a GPU ending in the library's error with nothing on stdout."""
import json
import os
import subprocess

import pytest

import convert_restate as cr
from convert_cases import FMT_EXT, OPS, seeded_lines

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
TOOL = os.path.join(CSRC, "genomic_convert")
REGIONS = os.path.join(CSRC, "genomic_regions")
GOLD = os.path.join(HERE, "golden")
CASES = json.load(open(os.path.join(GOLD, "convert_manifest.json")))["cases"]


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
    name = "in." + FMT_EXT[case["fmt"]]
    (tmp_path / name).write_text(text)
    want = (case["stdout"], case["stderr"], case["code"])
    assert tool(cr.tool_args(case["op"]) + [name], tmp_path) == want
    assert tool(cr.tool_args(case["op"]), tmp_path, stdin=text.encode()) == want


@pytest.mark.parametrize("fmt,op", [(f, o) for f in cr.FORMATS for o in OPS[f]], ids=lambda v: v if isinstance(v, str) else "-".join(cr.tool_args(v)).replace(",", "."))
def test_host_loop_equals_the_restatement_on_seeded_lines(tmp_path, fmt, op):
    text = seeded_lines(fmt, 11 + OPS[fmt].index(op))
    want = cr.run(op, text, fmt)
    assert want[1:] == ("", 0) and want[0].count("\n") >= 3000
    assert sum(not cr.is_plain(l, fmt) for l in text.split("\n")[:-1]) >= 1000
    name = "in." + FMT_EXT[fmt]
    (tmp_path / name).write_bytes(text.encode())
    assert tool(cr.tool_args(op) + [name], tmp_path) == want
    assert tool(cr.tool_args(op), tmp_path, stdin=text.encode()) == want


def test_usage_help_and_option_errors(tmp_path):
    out, err, rc = tool([], tmp_path)
    assert (out, rc) == ("", 1) and "genomic_convert OPERATION [OPTIONS] <REGION-SET>" in err
    assert "  bed        Converts input regions into BED format.\n" in err and "  reg        Converts to REG format.\n" in err
    assert tool(["wig", "a.sam"], tmp_path) == ("", "Unknown operation 'wig'!\n", 1)
    out, err, rc = tool(["bed", "-h"], tmp_path)
    assert (out, rc) == ("", 1) and "genomic_convert bed [OPTIONS] <REGION-SET>" in err
    for o, text in [("--help", "help"), ("-h", "help"), ("-v", "verbose mode"), ("-t", "title"), ("-c", "color"), ("-p", "browser position"),
                    ("-chr", "convert chromosome names from ENSEMBL to UCSC")]:
        assert "\n  %-25s %s\n" % (o, text) in err, o
    assert "Converts input regions into BED format." in err and "Region requirements: chromosome/strand-compatible, sorted, non-overlapping" in err
    assert "--ngpu" not in err
    assert tool(["bed", "--help"], tmp_path) == (out, err, rc)
    out, err, rc = tool(["reg", "--help"], tmp_path)
    assert (out, rc) == ("", 1) and "genomic_convert reg [OPTIONS] <REGION-SET>" in err
    assert "\n  %-25s %s\n" % ("-c", "print in compact starts/ends format") in err and "-chr" not in err
    assert "Converts to REG format." in err and "Region requirements: chromosome/strand-compatible if option -c is set" in err
    assert tool(["bed", "--bogus", "a.sam"], tmp_path) == ("", "Error: unknown option '--bogus'!\n", 1)
    assert tool(["reg", "-chr", "a.sam"], tmp_path) == ("", "Error: unknown option '-chr'!\n", 1)
    assert tool(["bed", "--ngpu", "2", "a.sam"], tmp_path) == ("", "Error: unknown option '--ngpu'!\n", 1)
    assert tool(["bed", "-t"], tmp_path) == ("", "Error: could not set option '-t'!\n", 1)
    assert tool(["bed", "-c"], tmp_path) == ("", "Error: could not set option '-c'!\n", 1)


def test_bed_on_a_bed_set_is_refused_before_a_device_is_looked_for(tmp_path):
    (tmp_path / "a.bed").write_text("track name=x\nchr1\t0\t10\tlab\n")
    for host_loop in (True, False):
        out, err, rc = tool(["bed", "a.bed"], tmp_path, host_loop=host_loop)
        assert (out, rc) == ("", 1) and err == "Error: the bed operation takes SAM and GFF input: a BED set is not converted into BED!\n"


def test_a_bad_fragment_ends_the_run_behind_the_lines_in_front(tmp_path):
    want_err = open(os.path.join(GOLD, "g12_bad_fragment.err")).read()
    sam = os.path.join(GOLD, "g12_bad_fragment.sam")
    assert tool(["bed", sam], tmp_path) == ("chr1\t9\t14\tx1\t1000\t+\n", want_err, 1)
    assert tool(["reg", sam], tmp_path) == ("x1\tchr1 + 10 14\n", want_err, 1)
    assert cr.run({"to": "bed"}, open(sam).read(), "sam") == ("chr1\t9\t14\tx1\t1000\t+\n", want_err, 1)


def test_an_empty_set_prints_nothing(tmp_path):
    (tmp_path / "a.sam").write_text("")
    assert tool(["bed", "-t", "T", "a.sam"], tmp_path) == ("", "", 0)
    assert tool(["reg"], tmp_path, stdin=b"") == ("", "", 0)


def test_without_a_gpu_the_run_fails_with_the_librarys_error(tmp_path):
    """whatever the input's size the device is looked for: a run may not quietly take the host loop"""
    (tmp_path / "a.sam").write_text("r1\t0\tchr1\t100\t30\t10M\t*\t0\t0\t*\t*\n")
    for args, stdin in ((["bed", "-t", "T", "a.sam"], None), (["reg"], b"chr1\t0\t10\n"), (["bed"], b"chr1\tsrc\texon\t11\t20\t.\t+\t.\n")):
        out, err, rc = tool(args, tmp_path, stdin, host_loop=False)
        assert rc == 1 and out == ""
        assert "no usable HIP device" in err and "no CPU path" in err


def test_genomic_regions_still_refuses_both_words(tmp_path):
    for word in ("bed", "reg"):
        out, err, rc = tool([word, "a.bed"], tmp_path, exe=REGIONS)
        assert (out, rc) == ("", 1) and err == "Operation '%s' is outside the MI355X path of this build!\n" % word
