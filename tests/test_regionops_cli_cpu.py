"""genomic_regions shift | shiftp | pos | center | fix | bounds (csrc/genomic_regions.cpp) without a GPU: usage, help and option
errors with the reference's options (gtools/genomic_regions.cpp:497-499, :579-582, :606-613), the refusal of the reference's 26
other operations by name, the genome file of `bounds` (:693 with ReadBounds gtools/genomic_intervals.cpp:5997-6015), the operator
word of `pos`, and a run without a GPU ending in the library's error with nothing on stdout.  With GTX_TEXT_ON_DEVICE=0 the
operations run their host loop, which looks for no device."""
import os
import subprocess

import pytest

import regionops_restate as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_regions")

OPTIONS = {
    "shift": [("-start", "shift distance for start position"), ("-stop", "shift distance for stop position")],
    "shiftp": [("-5p", "shift distance for 5' end"), ("-3p", "shift distance for 3' end")],
    "pos": [("-op", "position operation (1=start, 2=stop, 5p=5'-end, 3p=3'-end, c=center)"), ("-c", "position shift")],
    "center": [], "fix": [],
    "bounds": [("-g", "genome region-set file")],
}
TEXTS = {
    "shift": "Shifts interval start/stop positions.", "shiftp": "Shifts interval 5'/3' positions.", "pos": "Modifies interval start/stop positions.",
    "center": "Prints center interval.", "fix": "Removes invalid intervals, i.e. start<1 or start>stop.",
    "bounds": "Trims start/stop positions given the chromosome bounds and removes invalid intervals.",
}
OTHERS = ["align", "annotator", "bed", "chrom", "connect", "diff", "dist", "divide", "int", "n", "reg", "rnd", "search", "select", "shuffle",
          "sort", "split", "strand", "union", "wig", "win", "x", "gdist", "gsort", "inv", "test"]


def tool(args, cwd, stdin=None, host_loop=False):
    assert os.path.exists(TOOL), "genomic_regions has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    env.pop("GTX_TEXT_ON_DEVICE", None)
    if host_loop:
        env["GTX_TEXT_ON_DEVICE"] = "0"
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd, env=env, input=stdin)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


@pytest.mark.parametrize("op", sorted(OPTIONS))
def test_help_lists_the_options(tmp_path, op):
    rc, out, err = tool([op, "-h"], tmp_path)
    assert rc == 1 and out == ""
    assert "genomic_regions %s [OPTIONS] <REGION-SET>" % op in err
    for o, text in [("--help", "help"), ("-h", "help"), ("-v", "verbose mode")] + OPTIONS[op]:
        assert "\n  %-25s %s\n" % (o, text) in err, o
    assert TEXTS[op] in err and "Input formats: BED" in err and "Operand: interval" in err
    assert "--ngpu" not in err
    assert tool([op, "--help"], tmp_path) == (1, "", err)
    assert tool([op, "-h", "nothing.bed"], tmp_path) == (1, "", err)


def test_no_operation_lists_the_seven(tmp_path):
    rc, out, err = tool([], tmp_path)
    assert rc == 1 and out == "" and "USAGE" in err
    for op in list(OPTIONS) + ["link"]:
        assert "\n  %-10s " % op in err, op
    for op in OPTIONS:
        assert TEXTS[op] in err


@pytest.mark.parametrize("op", sorted(OPTIONS))
def test_option_errors(tmp_path, op):
    assert tool([op, "--bogus", "a.bed"], tmp_path) == (1, "", "Error: unknown option '--bogus'!\n")
    assert tool([op, "--ngpu", "2", "a.bed"], tmp_path) == (1, "", "Error: unknown option '--ngpu'!\n")
    assert tool([op, "-d", "5", "a.bed"], tmp_path) == (1, "", "Error: unknown option '-d'!\n")          # link's, not theirs
    for o, _ in OPTIONS[op]:
        assert tool([op, o], tmp_path) == (1, "", "Error: could not set option '%s'!\n" % o)
    for other, opts in OPTIONS.items():                                                                  # an option of another operation
        for o, _ in opts:
            if o not in [x for x, _ in OPTIONS[op]]:
                assert tool([op, o, "1", "a.bed"], tmp_path) == (1, "", "Error: unknown option '%s'!\n" % o)


def test_the_other_26_operations_are_still_refused_by_name(tmp_path):
    assert len(OTHERS) == 26
    for op in OTHERS:
        rc, out, err = tool([op, "nothing.bed"], tmp_path)
        assert rc == 1 and out == ""
        assert err.startswith("Operation '%s' is outside the MI355X path of this build" % op) and err.count("\n") == 1
    assert tool(["Shift", "a.bed"], tmp_path) == (1, "", "Unknown operation 'Shift'!\n")


LINES = "chr1\t149\t300\tx\nchr1\t150\t300\tx\nchr1\t-5\t1\tx\nchrX\t1\t2\tx\nchr1 10 20 x 3 .\n"


def test_bounds_and_its_genome_file(tmp_path):
    (tmp_path / "a.bed").write_text(LINES)
    (tmp_path / "g.bed").write_text("chr1\t0\t150\nchr2\t0\t99\nchr1\t0\t150\n")
    (tmp_path / "g2.bed").write_text("chr1\t0\t150\nchr1\t0\t151\n")
    # :693 with ReadBounds: without -g the run ends before the set is opened
    assert tool(["bounds", "a.bed"], tmp_path) == (1, "", "Error: genome region file is necessary for this operation!\n")
    assert tool(["bounds", "-g", "", "a.bed"], tmp_path) == (1, "", "Error: genome region file is necessary for this operation!\n")
    assert tool(["bounds", "-g", "g2.bed", "a.bed"], tmp_path) == (1, "", "Error: chromosome chr1 has multiple lengths in genome file 'g2.bed' line 2!\n")
    want = rr.run({"kind": "bounds", "genome": {"chr1": 150, "chr2": 99}}, LINES)
    assert want == ("chr1\t149\t150\tx\nchr1\t0\t1\tx\nchr1\t10\t20\tx\t3\t+\n", "", 0)
    assert tool(["bounds", "-g", "g.bed", "a.bed"], tmp_path, host_loop=True) == (0,) + want[:2]
    assert tool(["bounds", "-g", "g.bed"], tmp_path, stdin=LINES.encode(), host_loop=True) == (0,) + want[:2]


def test_pos_operator_words(tmp_path):
    text = "track name=t\nchr1\t10\t20\ta\t5\t+\nchr1\t100\t200\tb\t7\t-\n"
    (tmp_path / "a.bed").write_text(text)
    for w in rr.POS_OPS:
        out, err, code = rr.run({"kind": "pos", "op": w, "c": 10}, text)
        assert tool(["pos", "-op", w, "-c", "10", "a.bed"], tmp_path, host_loop=True) == (code, out, err)
    # a word that is none of the five: RunModifyPos' error (:4081), behind the header the open set has echoed
    assert tool(["pos", "-op", "x", "a.bed"], tmp_path, host_loop=True) == (1, "track name=t\n", "Error: unknown operation!\n")
    assert tool(["pos", "a.bed"], tmp_path, host_loop=True)[1] == rr.run({"kind": "pos", "op": "1", "c": 0}, text)[0]     # the defaults: -op 1 -c 0


def test_the_host_loop_of_every_operation_and_an_input_error(tmp_path):
    text = "chr1\t10\t20\ta\t5\t+\nchr1\t100\t200\tb\t7\t-\nchr2\t0\t5\nchr1\t5\n"
    (tmp_path / "a.bed").write_text(text)
    for args, op in ((["shift", "-start", "5", "-stop", "-3"], {"kind": "shift", "a": 5, "b": -3}), (["shiftp", "-5p", "5", "-3p", "-3"], {"kind": "shiftp", "a": 5, "b": -3}),
                     (["center"], {"kind": "center"}), (["fix"], {"kind": "fix"})):
        out, err, code = rr.run(op, text)
        assert code == 1 and "Line 4" in err and out.count("\n") == 3
        assert tool(args + ["a.bed"], tmp_path, host_loop=True) == (code, out, err)


def test_a_set_that_is_not_bed_is_unsupported(tmp_path):
    (tmp_path / "a.sam").write_text("@HD\tVN:1.0\nr1\t0\tchr1\t5\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n")
    (tmp_path / "g.bed").write_text("chr1\t0\t150\n")
    for op in sorted(OPTIONS):
        rc, out, err = tool([op] + (["-g", "g.bed"] if op == "bounds" else []) + ["a.sam"], tmp_path, host_loop=True)
        assert rc == 1 and out == "" and "unsupported input format!" in err


def test_without_a_gpu_the_run_fails_with_the_librarys_error(tmp_path):
    (tmp_path / "a.bed").write_text("chr1\t0\t10\ta\nchr1\t5\t20\tb\n")
    (tmp_path / "g.bed").write_text("chr1\t0\t15\n")
    for args, stdin in ((["shift", "-start", "1", "a.bed"], None), (["shiftp", "-5p", "1"], b"chr1\t0\t10\t1\n"), (["pos", "-op", "c", "a.bed"], None),
                        (["center", "a.bed"], None), (["fix", "a.bed"], None), (["bounds", "-g", "g.bed", "a.bed"], None)):
        rc, out, err = tool(args, tmp_path, stdin)
        assert rc == 1 and out == ""
        assert "no usable HIP device" in err and "no CPU path" in err
