"""genomic_peakdiff (csrc/genomic_peakdiff.cpp: scans kept in HBM, windows selected on the device) against the restatement of the
reference's data pass (tests/peakdiff_restate.py), byte for byte on PREFIX.dat and PREFIX.params: the hand-derived vectors of
tests/golden/peakdiff_manifest.json, and generated inputs of a few thousand reads each in which the restatement keeps some windows
and not all."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import peakdiff_restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_peakdiff")
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "peakdiff_manifest.json")))
NOTE = "Plot step skipped: this build writes the .dat and .params files only (no R script is written or run).\n"


def tool(args, cwd, env=None):
    assert os.path.exists(TOOL), "genomic_peakdiff has not been built (make -C ibm-cbc-genomic-tools_amd/csrc)"
    e = dict(os.environ)
    for k in ("GTX_TEXT_ON_DEVICE", "GTX_TEXT_TRACE", "GTX_NGPU"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd, env=e)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def write(path, lines):
    with open(path, "w") as f:
        f.write("".join(l + "\n" for l in lines))


def lay_out(d, genome, groups):
    """the files of a run in directory d; returns the positional arguments (comma-separated names per group)"""
    write(d / "genome.bed", genome)
    args = []
    for tag, files in groups:
        if not files:
            continue
        names = []
        for k, lines in enumerate(files):
            names.append("%s%d.bed" % (tag, k + 1)); write(d / names[-1], lines)
        args.append(",".join(names))
    return args


def run_and_compare(d, genome, signal, ref, signal_control, ref_control, options, env=None):
    files = lay_out(d, genome, [("s", signal), ("r", ref), ("sc", signal_control), ("rc", ref_control)])
    args = ["-o", "out", "-labels", "A,B", "-g", "genome.bed"] + options + files
    rc, out, err = tool(args, d, env)
    assert (rc, out) == (0, ""), err
    assert err.endswith(NOTE)
    kw = peakdiff_restate.case_options(options)
    dat, n_windows, kept = peakdiff_restate.peakdiff_dat(genome, signal, ref, signal_control, ref_control, ["A", "B"], **kw)
    assert (d / "out.dat").read_text() == dat
    assert (d / "out.params").read_text() == peakdiff_restate.params_text([TOOL] + args, len(signal), len(ref), win_size=kw.get("win_size", 500),
                                                                          pval=kw.get("pval", 1e-5), labels="A,B")
    return dat, n_windows, kept, err


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_manifest_vectors(tmp_path, case):
    dat, _, _, err = run_and_compare(tmp_path, case["genome"], case["signal"], case["ref"], case["signal_control"], case["ref_control"], case["options"])
    assert dat == case["dat"] and err == NOTE


GENOME = [("chrA", 300000), ("chrB", 200050), ("chrC", 100499), ("chrD", 420)]        # chrD is shorter than a window
GENOME_LINES = ["%s\t0\t%d" % g for g in GENOME]


def reads(seed, n, hot=0.3, labels=None, shuffle=True, unknown=0):
    """n BED6 reads of 36 to 75 bp: a uniform background plus `hot` of them in thirty 300-bp hotspots (shared by every file of a run,
    with file-specific strengths), `unknown` more on a chromosome without bounds"""
    rng = np.random.default_rng(seed)
    spots = np.random.default_rng(99)
    hs = [(int(spots.integers(0, 3)), int(spots.integers(0, 90000))) for _ in range(30)]
    strength = rng.random(30) ** 3
    strength /= strength.sum()
    rows = []
    for i in range(n):
        if rng.random() < hot:
            c, at = hs[int(rng.choice(30, p=strength))]
            s = at + int(rng.integers(0, 300))
        else:
            c = int(rng.choice(3, p=[0.5, 0.33, 0.17])); s = int(rng.integers(0, GENOME[c][1] - 80))
        rows.append((GENOME[c][0], s, s + int(rng.integers(36, 76)), labels(rng) if labels else "r%d" % i, "+-"[int(rng.integers(0, 2))]))
    rows += [("chrUn", int(rng.integers(0, 1000)), 2000, "u", "+") for _ in range(unknown)]
    order = rng.permutation(len(rows)) if shuffle else sorted(range(len(rows)), key=lambda k: (rows[k][0], rows[k][1]))
    return ["%s\t%d\t%d\t%s\t0\t%s" % rows[k] for k in order]


GENERATED = {
    "1+1": dict(signal=[(1, 3000)], ref=[(2, 4000)], options=[]),
    "2+2": dict(signal=[(3, 3000), (4, 2500)], ref=[(5, 3500), (6, 2000)], options=["-pval", "1e-4"]),
    "2+2_controls": dict(signal=[(7, 3000), (8, 2500)], ref=[(9, 3500), (10, 2000)], control=True, options=["-pval", "1e-3"]),
    "1+1_controls_w200_d50": dict(signal=[(11, 5000)], ref=[(12, 4000)], control=True, options=["-w", "200", "-d", "50", "-pval", "1e-4"]),
}


def generated(name):
    g = GENERATED[name]
    signal, ref = [reads(s, n, unknown=5) for s, n in g["signal"]], [reads(s, n) for s, n in g["ref"]]
    sc = [reads(100 + s, n // 2, hot=0.15) for s, n in g["signal"]] if g.get("control") else []
    rc = [reads(100 + s, n // 2, hot=0.15) for s, n in g["ref"]] if g.get("control") else []
    return signal, ref, sc, rc, g["options"]


@pytest.mark.parametrize("strand", ["-i", "stranded"])
@pytest.mark.parametrize("name", list(GENERATED))
def test_generated_inputs(tmp_path, name, strand):
    signal, ref, sc, rc, options = generated(name)
    _, n_windows, kept, _ = run_and_compare(tmp_path, GENOME_LINES, signal, ref, sc, rc, options + (["-i"] if strand == "-i" else []))
    assert 0 < kept < n_windows                                      # an empty comparison cannot pass for a right one


def test_max_label_value_3_region_count_and_label_sum_differ(tmp_path):
    lab = lambda rng: str(int(rng.integers(0, 7)))
    signal, ref = [reads(21, 3000, labels=lab)], [reads(22, 3000, labels=lab)]
    options = ["-i", "--max-label-value", "3", "-pval", "1e-4"]
    _, n_windows, kept, _ = run_and_compare(tmp_path, GENOME_LINES, signal, ref, [], [], options)
    assert 0 < kept < n_windows
    # with the label sum in the background instead of the region count the output would differ: the case does tell them apart
    total = sum(min(3, int(l.split("\t")[3])) for l in signal[0])
    assert total != len(signal[0])


def test_sorted_input_gives_the_same_as_shuffled(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    da, _, kept, _ = run_and_compare(a, GENOME_LINES, [reads(31, 3000, shuffle=True)], [reads(32, 3000, shuffle=True)], [], [], ["-i"])
    db, _, _, _ = run_and_compare(b, GENOME_LINES, [reads(31, 3000, shuffle=False)], [reads(32, 3000, shuffle=False)], [], [], ["-i"])
    assert da == db and kept > 0


def test_text_tokenised_on_the_device_feeds_a_kept_scan(tmp_path):
    signal, ref, sc, rc, options = generated("2+2_controls")
    _, n_windows, kept, err = run_and_compare(tmp_path, GENOME_LINES, signal, ref, sc, rc, options, env={"GTX_TEXT_ON_DEVICE": "1", "GTX_TEXT_TRACE": "1"})
    assert 0 < kept < n_windows
    traces = re.findall(r"\[gtx text\] blocks tokenised on the device: (\d+), sent back to the host packer: (\d+)", err)
    assert len(traces) >= 8 and all(int(a) >= 1 and int(b) == 0 for a, b in traces)


def test_verbose_lines(tmp_path):
    signal, ref = [reads(41, 600)], [reads(42, 300)]
    files = lay_out(tmp_path, GENOME_LINES, [("s", signal), ("r", ref)])
    rc, out, err = tool(["-v", "-o", "out", "-labels", "A,B", "-g", "genome.bed", "-i"] + files, tmp_path)
    assert rc == 0
    genome = sum(n for _, n in GENOME)
    assert "* Effective genome size = %d\n" % genome in err
    assert "* Signal input file = s1.bed; background probability = %.2e\n" % (600 / genome) in err
    assert "* Reference input file = r1.bed; background probability = %.2e\n" % (300 / genome) in err


def test_background_probability_above_one_is_an_error(tmp_path):
    files = lay_out(tmp_path, ["chrA\t0\t2"], [("s", [["chrA\t0\t1", "chrA\t0\t1", "chrA\t1\t2"]]), ("r", [["chrA\t0\t1"]])])
    rc, out, err = tool(["-o", "out", "-labels", "A,B", "-g", "genome.bed", "-w", "2", "-d", "2"] + files, tmp_path)
    assert (rc, out) == (1, "")
    assert err == "Error: background probability of 's1.bed' is above 1: 3 regions on 2 genome positions!\n"


def test_bounds_without_a_window_give_the_header_alone(tmp_path):
    dat, n_windows, kept, _ = run_and_compare(tmp_path, ["chrA\t0\t3"], [["chrA\t0\t2"]], [["chrA\t1\t3"]], [], [], ["-i", "-w", "4", "-d", "2", "-pval", "1.0"])
    assert (n_windows, kept) == (0, 0) and dat == "locus\tA count 1\tB count 1\n"


def test_more_than_one_gpu_is_an_error_the_tool_prints(tmp_path):
    files = lay_out(tmp_path, GENOME_LINES, [("s", [reads(51, 200)]), ("r", [reads(52, 200)])])
    rc, out, err = tool(["-o", "out", "-labels", "A,B", "-g", "genome.bed"] + files, tmp_path, env={"GTX_NGPU": "2", "GTX_GROUP_REHEARSE": "1"})
    assert (rc, out) == (1, "") and "one GPU only" in err
