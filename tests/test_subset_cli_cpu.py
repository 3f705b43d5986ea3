"""genomic_subset (csrc/genomic_subset.cpp) without a GPU: the usage with the reference's options for `subset`
(gtools/genomic_overlaps.cpp:185-191, :246-249) and the argument errors that come before any region file is read -- the -S -s -i
refusal with the reference's text and exit status 1 (:305), the option parser's own (core.cpp:2420-2436)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_subset")

SSI = ("[Error]: the input is sorted by chromosome/strand/start (i.e. -S and -s are set), therefore the overlap algorithm can only "
       "report strand-specific results (i.e. -i cannot be set)!\n")


def tool(args, cwd):
    assert os.path.exists(TOOL), "genomic_subset has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)"
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_usage_lists_the_options(tmp_path):
    rc, out, err = tool([], tmp_path)
    assert rc == 1 and out == ""
    assert "genomic_subset [OPTIONS] REFERENCE-REGION-FILE <TEST-REGION-FILE>" in err
    for o in ["-inv", "-gaps", "-S", "-s", "-i", "-B", "-v", "-h", "--help"]:
        assert "\n  %s " % o in err, o
    for args in (["-h"], ["--help"], ["-h", "a.bed", "b.bed"], ["-inv", "-S"]):   # help, or no reference file
        assert tool(args, tmp_path) == (1, "", err), args


def test_sorted_by_strand_cannot_ignore_the_strand(tmp_path):
    """before any file is opened: the files named do not exist"""
    for args in (["-S", "-s", "-i"], ["-i", "-inv", "-s", "-gaps", "-S"]):
        assert tool(args + ["no_refs.bed", "no_reads.bed"], tmp_path) == (1, "", SSI)
        assert tool(args + ["no_refs.bed"], tmp_path) == (1, "", SSI)


def test_option_errors(tmp_path):
    assert tool(["--bogus", "a.bed", "b.bed"], tmp_path) == (1, "", "Error: unknown option '--bogus'!\n")
    assert tool(["--max-label-value", "3", "a.bed", "b.bed"], tmp_path) == (1, "", "Error: unknown option '--max-label-value'!\n")   # not an option of subset
    assert tool(["-label", "a.bed", "b.bed"], tmp_path) == (1, "", "Error: unknown option '-label'!\n")
    assert tool(["-B"], tmp_path) == (1, "", "Error: could not set option '-B'!\n")


def test_the_operation_word_is_not_taken(tmp_path):
    """the tool takes the reference's command line BEHIND the operation word: `subset` itself reads as the reference file"""
    (tmp_path / "r.bed").write_text("chr1\t150\t160\tA\t0\t+\n")
    rc, out, err = tool(["subset", "r.bed"], tmp_path)
    assert rc == 1 and out == "" and "subset" in err and "USAGE" not in err
