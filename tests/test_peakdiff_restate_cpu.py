"""CPU suite: the Python restatement of peakdiff's data pass (tests/peakdiff_restate.py) against hand-derived vectors
(tests/golden/peakdiff_manifest.json, each marked `derived` with the reference lines it follows and the tails worked out by hand)."""
import json
import os

import pytest

import peakdiff_restate

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "peakdiff_manifest.json")))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_hand_derived_output(case):
    assert case["derived"] and case["cites"]
    dat, n_windows, kept = peakdiff_restate.peakdiff_dat(case["genome"], case["signal"], case["ref"], case["signal_control"], case["ref_control"], ["A", "B"],
                                                         **peakdiff_restate.case_options(case["options"]))
    assert dat == case["dat"]
    assert kept == case["dat"].count("\n") - 1 and kept <= n_windows


def test_manifest_covers_what_the_issue_lists():
    by = {c["name"]: c for c in CASES}
    assert any("-i" in c["options"] for c in CASES) and any("-i" not in c["options"] for c in CASES)
    assert any(len(c["signal"]) == 1 and len(c["ref"]) == 1 for c in CASES) and any(len(c["signal"]) == 2 and len(c["ref"]) == 2 for c in CASES)
    assert any(c["signal_control"] for c in CASES) and any(len(c["signal_control"]) == 2 for c in CASES)
    for word in ("controls_lift_p", "clamp", "cutoff_one", "second_sample_only", "max_label_value"):
        assert any(word in n for n in by), word
    assert all(len(f) <= 12 for c in CASES for k in ("signal", "ref", "signal_control", "ref_control") for f in c[k])
    assert all(1 <= len(c["genome"]) <= 2 for c in CASES)


def test_params_text():
    t = peakdiff_restate.params_text(["tool", "-o", "x", "-labels", "A,B", "two words", "b"], 1, 2, labels="A,B")
    assert t == ("n_signal 1\nn_ref 2\nwin 500\npval 1.000000e-05\nscale winsize\nnorm normq\npseudo 1.000000e+00\noutliers 1.000000e-02\nfdr 5.000000e-02\n"
                 "fold 1.000000e+00\nfdr_bins 1\nlabels A,B\nisize 3000,2000\nires 300\n# tool -o x -labels A,B 'two words' b\n")


def test_background_above_one_is_refused():
    with pytest.raises(peakdiff_restate.BackgroundAboveOne):
        peakdiff_restate.peakdiff_dat(["chrA\t0\t2"], [["chrA\t0\t1", "chrA\t0\t1", "chrA\t1\t2"]], [["chrA\t0\t1"]], [], [], ["A", "B"], win_size=2, win_dist=2)
