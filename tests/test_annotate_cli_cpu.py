"""CPU suite: genomic_annotate's command line (csrc/genomic_annotate.cpp) where no GPU is needed -- the usage, the option parser's
errors, the -S -s -i error, and a multi-interval reference file refused by the upstream builder before any output.  Run with
HIP_VISIBLE_DEVICES=-1 so that nothing here can reach a device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_annotate")
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="-1")

OPTIONS = ["--help", "-h", "-v", "-B", "-S", "-s", "-i", "--query-op", "--upstream-max", "--upstream-min", "--distance-flag", "--proximal-dist", "--print-header"]


def tool(args, cwd=None):
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd, env=ENV)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_usage_lists_every_option():
    for args in ([], ["-h"], ["--help"], ["-i", "--distance-flag"]):
        rc, out, err = tool(args)
        assert rc == 1 and out == ""
        assert err.startswith("\nUSAGE: \n  genomic_annotate [OPTIONS] REFERENCE-REGION-FILE <TEST-REGION-FILE>\n\nOPTIONS: \n")
        listed = [l.split()[0] for l in err.splitlines() if l.startswith("  -")]
        assert listed == OPTIONS


def test_sorted_by_strand_and_ignore_strand_is_the_error_before_any_file_is_opened():
    rc, out, err = tool(["-S", "-s", "-i", "no_such_refs.bed", "no_such_tests.bed"])
    assert (rc, out) == (1, "")
    assert err.startswith("[Error]: the input is sorted by chromosome/strand/start (i.e. -S and -s are set)") and err.endswith("(i.e. -i cannot be set)!\n")


def test_option_parser_errors():
    assert tool(["-gaps", "r.bed"]) == (1, "", "Error: unknown option '-gaps'!\n")
    assert tool(["--upstream-max"]) == (1, "", "Error: could not set option '--upstream-max'!\n")
    assert tool(["--distance-flag", "--query-op"]) == (1, "", "Error: could not set option '--query-op'!\n")


def test_multi_interval_reference_file_is_refused_before_any_output(tmp_path):
    (tmp_path / "r.bed").write_text("chr1\t1000\t2000\tG\t0\t+\nchr1\t3000\t4000\tM\t0\t+\t3000\t4000\t0\t2\t100,100,\t0,900,\n")
    (tmp_path / "t.bed").write_text("chr1\t1000\t1002\tt1\t0\t+\n")
    msg = "\nError: Line 2: single-interval reference regions are required for this operation!\n"
    assert tool(["--print-header", "r.bed", "t.bed"], tmp_path) == (1, "", msg)
    assert tool(["--print-header", "-S", "--upstream-max", "1", "--upstream-min", "0", "r.bed", "t.bed"], tmp_path) == (1, "", msg)
    # overlapping blocks: the reference's index refuses the region first (its constructor's check)
    (tmp_path / "r2.bed").write_text("chr1\t3000\t4000\tM\t0\t+\t3000\t4000\t0\t2\t600,500,\t0,500,\n")
    assert tool(["r2.bed", "t.bed"], tmp_path) == (1, "", "\nError: Line 1: index regions should be compatible, sorted and non-overlapping!\n")


def test_sam_is_refused(tmp_path):
    (tmp_path / "r.bed").write_text("chr1\t1000\t2000\tG\t0\t+\n")
    (tmp_path / "t.sam").write_text("r1\t0\tchr1\t1001\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n")
    rc, out, err = tool(["r.bed", "t.sam"], tmp_path)
    assert (rc, out) == (1, "") and "unsupported input format!" in err
