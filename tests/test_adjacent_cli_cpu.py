"""genomic_adjacent (csrc/genomic_adjacent.cpp) without a GPU: the usage of `inv`, `gdist` and `test` with the reference's options
(gtools/genomic_regions.cpp:413-419, :429-435, :445-451, :525-528, :536-538, :627-629), the unknown-operation message (:660), a SAM
file refused, ReadBounds' error for `inv` without -g, an empty file, and a run without a GPU ending in the library's error with nothing
on stdout."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_adjacent")
COMMON = [("--help", "help"), ("-h", "help"), ("-v", "verbose mode")]
POINT = "reference point of %s interval in pair (1=start, 2=stop, 5p=5'-end, 3p=3'-end)"


def tool(args, cwd, stdin=None):
    assert os.path.exists(TOOL), "genomic_adjacent has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)"
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), input=stdin)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def usage_lists(err, op, options, about, needs):
    assert "genomic_adjacent %s [OPTIONS] <REGION-SET>" % op in err
    for o, text in COMMON + options:
        assert "\n  %-25s %s\n" % (o, text) in err, o
    assert about in err and needs in err


def test_usage_of_each_operation_lists_its_options(tmp_path):
    for op, options, about, needs in (
            ("inv", [("-g", "genome region-set file")], "Inverts regions given the genome chromosomal boundaries.", "sorted by chromosome/strand/start"),
            ("gdist", [("-op1", POINT % "1st"), ("-op2", POINT % "2nd")], "Computes distances of successive regions.", "Operand: region-pair"),
            ("test", [("-s", "input regions are sorted by strand")], "Tests whether genomic regions are sorted and non-overlapping.",
             "sorted by chromosome/(strand)/start")):
        rc, out, err = tool([op, "-h"], tmp_path)
        assert rc == 1 and out == ""
        usage_lists(err, op, options, about, needs)
        assert tool([op, "--help"], tmp_path) == (1, "", err)
        assert tool([op, "-v", "-h", "nothing.bed"], tmp_path) == (1, "", err)
    assert "-s " not in tool(["inv", "-h"], tmp_path)[2] and "-g " not in tool(["test", "-h"], tmp_path)[2]


def test_no_operation_lists_the_three(tmp_path):
    rc, out, err = tool([], tmp_path)
    assert rc == 1 and out == "" and "USAGE" in err
    for op in ("gdist", "inv", "test"):
        assert "\n  %s " % op in err


def test_unknown_operation(tmp_path):
    assert tool(["link", "nothing.bed"], tmp_path) == (1, "", "Unknown operation 'link'!\n")
    assert tool(["Inv"], tmp_path) == (1, "", "Unknown operation 'Inv'!\n")
    assert tool(["gsort", "a.bed"], tmp_path) == (1, "", "Unknown operation 'gsort'!\n")


def test_option_errors(tmp_path):
    assert tool(["test", "--bogus", "a.bed"], tmp_path) == (1, "", "Error: unknown option '--bogus'!\n")
    assert tool(["inv", "-s", "a.bed"], tmp_path) == (1, "", "Error: unknown option '-s'!\n")           # not an option of inv
    assert tool(["gdist", "-g", "x", "a.bed"], tmp_path) == (1, "", "Error: unknown option '-g'!\n")
    assert tool(["gdist", "-op1"], tmp_path) == (1, "", "Error: could not set option '-op1'!\n")


def test_inv_without_a_genome_file_gives_readbounds_error(tmp_path):
    (tmp_path / "a.bed").write_text("chr1\t0\t10\ta\n")
    assert tool(["inv", "a.bed"], tmp_path) == (1, "", "Error: genome region file is necessary for this operation!\n")


def test_a_sam_file_is_refused(tmp_path):
    (tmp_path / "in.sam").write_text("@HD\tVN:1.0\nr1\t0\tchr1\t100\t30\t50M\t*\t0\t0\t*\t*\n")
    (tmp_path / "g.bed").write_text("chr1\t0\t1000\n")
    for args in (["test", "in.sam"], ["gdist", "in.sam"], ["inv", "-g", "g.bed", "in.sam"]):
        rc, out, err = tool(args, tmp_path)
        assert rc == 1 and out == "" and err.endswith("Error: unsupported input format!\n\n")


def test_an_empty_file_prints_nothing_and_needs_no_device(tmp_path):
    (tmp_path / "empty.bed").write_text("")
    (tmp_path / "header.bed").write_text("track name=x\n")
    (tmp_path / "g.bed").write_text("chr1\t0\t1000\n")
    for args in (["test"], ["test", "-s"], ["gdist"], ["inv", "-g", "g.bed"]):
        assert tool(args + ["empty.bed"], tmp_path) == (0, "", "")
        assert tool(args + ["header.bed"], tmp_path) == (0, "track name=x\n", "")


def test_without_a_gpu_the_run_fails_with_the_librarys_error(tmp_path):
    (tmp_path / "a.bed").write_text("chr1\t0\t10\ta\nchr1\t5\t20\tb\n")
    (tmp_path / "g.bed").write_text("chr1\t0\t1000\n")
    for args, stdin in ((["test", "a.bed"], None), (["gdist", "-op2", "2"], b"chr1\t0\t10\t1\n"), (["inv", "-g", "g.bed", "a.bed"], None)):
        rc, out, err = tool(args, tmp_path, stdin)
        assert rc == 1 and out == ""
        assert "no usable HIP device" in err and "no CPU path" in err
