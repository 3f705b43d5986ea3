"""genomic_overlaps offset on the command line without a GPU: the operation is offered (its usage, with the reference's options,
instead of the refusal), and -S --skip-ref-gaps is the reference's error (gtools/genomic_overlaps.cpp:587-590) before any file
is opened.  The other operations outside the path keep their refusal."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_overlaps")


def tool(args, cwd):
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_offset_usage_lists_its_options(tmp_path):
    rc, out, err = tool(["offset", "-h"], tmp_path)
    text = out + err
    assert rc == 1
    assert "outside the MI355X" not in text
    assert "genomic_overlaps offset [OPTIONS] REFERENCE-REGION-FILE <TEST-REGION-FILE>" in text
    for opt in ("-op", "--skip-ref-gaps", "-label", "-gaps", "-a", "-c", "-S", "-s", "-i", "-B"):
        assert "\n  %s " % opt in text, opt
    assert "reference point (1=start, 2=stop, 5p=5'-end, 3p=3'-end)" in text


def test_offset_is_listed_among_the_operations(tmp_path):
    rc, _, err = tool([], tmp_path)
    assert rc == 1 and "\n  offset     " in err


def test_sorted_skip_ref_gaps_is_the_reference_error(tmp_path):
    # no such files: the error comes before either set is opened
    rc, out, err = tool(["offset", "-S", "--skip-ref-gaps", "missing_refs.bed", "missing_tests.bed"], tmp_path)
    assert (rc, out) == (1, "")
    assert err == "Error: option --subtract-gaps is not implemented for the -S option. Simply drop the -S and re-run!\n"


@pytest.mark.parametrize("op", ["annotate", "bin", "dist", "subset"])
def test_the_other_operations_stay_refused(tmp_path, op):
    rc, out, err = tool([op, "r.bed", "q.bed"], tmp_path)
    assert (rc, out) == (1, "")
    assert err == "Operation '%s' is outside the MI355X counting path of this build (count, coverage, density, rpkm)!\n" % op
