"""genomic_regions (csrc/genomic_regions.cpp) without a GPU: the usage of `link` with the reference's options
(gtools/genomic_regions.cpp:437-451, :469-471, :546-550), the refusal of the reference's other operations by name, the
unknown-operation message (:660), and a run without a GPU ending in the library's error with nothing on stdout."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_regions")


def tool(args, cwd, stdin=None):
    assert os.path.exists(TOOL), "genomic_regions has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)"
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), input=stdin)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_usage_of_link_lists_the_options(tmp_path):
    rc, out, err = tool(["link", "-h"], tmp_path)
    assert rc == 1 and out == ""
    assert "genomic_regions link [OPTIONS] <REGION-SET>" in err
    for o, text in [("--help", "help"), ("-h", "help"), ("-v", "verbose mode"), ("-s", "input regions are sorted by strand"),
                    ("-d", "maximum difference between successive regions"),
                    ("--label-func", "label function = {min,max,sum,%c}, where %c is used as delimiter")]:
        assert "\n  %-25s %s\n" % (o, text) in err, o
    assert "Links consecutive regions to produce a non-overlapping set." in err
    assert "sorted by chromosome/(strand)/start" in err
    assert tool(["link", "--help"], tmp_path) == (1, "", err)
    assert tool(["link", "-d", "5", "-h", "nothing.bed"], tmp_path) == (1, "", err)


def test_no_operation_lists_link(tmp_path):
    rc, out, err = tool([], tmp_path)
    assert rc == 1 and out == "" and "USAGE" in err and "\n  link " in err


def test_other_operations_are_refused_by_name(tmp_path):
    for op in ("inv", "gdist", "test", "union", "gsort"):
        rc, out, err = tool([op, "nothing.bed"], tmp_path)
        assert rc == 1 and out == ""
        assert err.startswith("Operation '%s' is outside the MI355X path of this build" % op) and err.count("\n") == 1


def test_unknown_operation(tmp_path):
    assert tool(["merge", "nothing.bed"], tmp_path) == (1, "", "Unknown operation 'merge'!\n")
    assert tool(["Link"], tmp_path) == (1, "", "Unknown operation 'Link'!\n")


def test_option_errors(tmp_path):
    assert tool(["link", "--bogus", "a.bed"], tmp_path) == (1, "", "Error: unknown option '--bogus'!\n")
    assert tool(["link", "-S", "a.bed"], tmp_path) == (1, "", "Error: unknown option '-S'!\n")          # not an option of link
    assert tool(["link", "-d"], tmp_path) == (1, "", "Error: could not set option '-d'!\n")


def test_without_a_gpu_the_run_fails_with_the_librarys_error(tmp_path):
    (tmp_path / "a.bed").write_text("chr1\t0\t10\ta\nchr1\t5\t20\tb\n")
    for args, stdin in ((["link", "a.bed"], None), (["link", "--label-func", "sum"], b"chr1\t0\t10\t1\n")):
        rc, out, err = tool(args, tmp_path, stdin)
        assert rc == 1 and out == ""
        assert "no usable HIP device" in err and "no CPU path" in err
