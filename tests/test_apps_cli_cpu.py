"""genomic_apps (csrc/genomic_apps.cpp) without a GPU: usage, the refused operations, and every argument error of
gtools/genomic_apps.cpp:95-240 / :466-540 / :752-800 with its exact text and exit status 1 -- all of them come before any
region file is read, so no GPU is involved."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_apps")


def tool(args, cwd):
    assert os.path.exists(TOOL), "genomic_apps has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)"
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    return r.returncode, r.stdout.decode(), r.stderr.decode()


@pytest.fixture
def d(tmp_path):
    (tmp_path / "s.bed").write_text("chr1\t100\t200\t1\t0\t+\n")
    (tmp_path / "r.bed").write_text("chr1\t150\t160\tA\t0\t+\n")
    return tmp_path


def test_usage_lists_the_options(d):
    rc, out, err = tool([], d)
    assert rc == 1 and "profile" in err and "heatmap" in err
    for op, only in (("profile", ["--norm-by-ref-regions", "-legend"]), ("heatmap", ["--nbins-smooth"])):
        rc, out, err = tool([op], d)
        assert rc == 1 and out == ""
        for o in ["-reuse", "-R", "-o", "-i", "--skip-ref-gaps", "--max-label-value", "--norm-ref-length", "--norm-by-total-reads",
                  "--norm-by-bin-size", "--bin-size", "-nbins", "-shift", "-colors", "-title", "-xlab", "-ylab", "-itype", "-isize", "-ires"] + only:
            assert "\n  %s " % o in err, (op, o)
        rc2, _, err2 = tool([op, "--help", "a", "b"], d)
        assert (rc2, err2) == (1, err)


def test_refused_operations(d):
    rc, out, err = tool(["peakdiff", "-o", "x", "a,b", "c,d"], d)
    assert rc == 1 and err.startswith("Operation 'peakdiff' is outside the MI355X path of this build")
    assert tool(["annotate", "s.bed", "r.bed"], d) == (1, "", "Unknown operation 'annotate'!\n")
    assert tool(["-profile", "s.bed", "r.bed"], d) == (1, "", "Unknown operation '-profile'!\n")


P = ["-colors", "red", "-legend", "L"]
H = ["-colors", "red", "-title", "T"]
ERRORS = [
    (["profile", "-o", "x", "-itype", "png"] + P, "Error: unsupported image format 'png'!\n"),
    (["heatmap", "-itype", "jpg"], "Error: unsupported image format 'jpg'!\n"),
    (["profile"] + P, "Error: prefix for output files must be specified using the -o option!\n"),
    (["heatmap"] + H, "Error: prefix for output files must be specified using the -o option!\n"),
    (["profile", "-o", "x", "-legend", "L"], "Error: number of colors must match total number of lines in the plot!\n"),
    (["profile", "-o", "x", "-colors", "a,b", "-legend", "L"], "Error: number of colors must match total number of lines in the plot!\n"),
    (["profile", "-o", "x", "-colors", "a"], "Error: number of legend labels must match total number of lines in the plot!\n"),
    (["heatmap", "-o", "x", "-title", "T"], "Error: number of colors must match number of signal files!\n"),
    (["heatmap", "-o", "x", "-colors", "a"], "Error: number of titles must match number of signal files!\n"),
    (["profile", "-o", "x", "--norm-ref-length", "--bin-size", "1.5"] + P, "Error: bin size cannot be greater than 1 when --norm-ref-length is set!\n"),
    (["heatmap", "-o", "x", "--norm-ref-length", "--bin-size", "2"] + H, "Error: bin size cannot be greater than 1 when --norm-ref-length is set!\n"),
    (["heatmap", "-o", "x", "--nbins-smooth", "100"] + H, "Error: number of bins to combine cannot be greater than total number of bins!\n"),
    (["heatmap", "-o", "x", "-nbins", "10", "--nbins-smooth", "12"] + H, "Error: number of bins to combine cannot be greater than total number of bins!\n"),
    (["profile", "-o", "x", "-R", "nope.r"] + P, "Error: R script file 'nope.r' not found!\n"),
    (["heatmap", "-o", "x", "-R", "nope.r"] + H, "Error: R script file 'nope.r' not found!\n"),
    (["profile", "-o", "x", "-nbins"], "Error: could not set option '-nbins'!\n"),
    (["profile", "-o", "x", "--bogus"] + P, "Error: unknown option '--bogus'!\n"),
]


@pytest.mark.parametrize("args,msg", ERRORS, ids=[" ".join(a) for a, _ in ERRORS])
def test_argument_errors(d, args, msg):
    rc, out, err = tool(args + ["s.bed", "r.bed"] if args[-1] != "-nbins" else args, d)
    assert (rc, out, err) == (1, "", msg)


def test_heatmap_takes_one_reference_file(d):
    assert tool(["heatmap", "-o", "x"] + H + ["s.bed", "r.bed,r.bed"], d) == (1, "", "Error: only one reference file allowed!\n")


def test_params_are_written_before_the_late_checks(d):
    """heatmap writes PREFIX.params before the -R and bin checks, profile before the -R check only (:485-500, :800-812)"""
    rc, _, _ = tool(["heatmap", "-o", "h", "--nbins-smooth", "100"] + H + ["s.bed", "r.bed"], d)
    assert rc == 1
    argv = " ".join([TOOL, "heatmap", "-o", "h", "--nbins-smooth", "100"] + H + ["s.bed", "r.bed"])
    assert (d / "h.params").read_text() == "5000\n5000\nred\nT\n\n\n2000,4000\n600\n1\n" + argv + "\n"
    assert not (d / "h.dat").exists()
    rc, _, _ = tool(["profile", "-o", "p", "-R", "nope.r", "-shift", "100.5,20", "-ylab", "two words"] + P + ["s.bed", "r.bed"], d)
    assert rc == 1
    argv = " ".join([TOOL, "profile", "-o", "p", "-R", "nope.r", "-shift", "100.5,20", "-ylab", "'two words'"] + P + ["s.bed", "r.bed"])
    assert (d / "p.params").read_text() == "-100.500000\n20.000000\nL\nred\n\n\ntwo words\n2000,2000\n300\n" + argv + "\n"
    rc, _, _ = tool(["profile", "-o", "q", "--norm-ref-length", "--bin-size", "2"] + P + ["s.bed", "r.bed"], d)
    assert rc == 1 and not (d / "q.params").exists()
