"""CPU suite: the numpy restatement of the peak candidate selection (tests/peaks_select_restate.py) against vectors derived by hand
(tests/golden/peaks_select_manifest.json, each with its derivation) -- the yardstick the device selection
(tests/test_gpu_peak_select.py) and `genomic_scans peaks` (tests/test_gpu_peaks_cli.py) are held to."""
import json
import os

import numpy as np
import pytest

import peaks_select_restate as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "peaks_select_manifest.json")))["cases"]


def vec(v):
    return None if v is None else np.array(v, dtype=np.uint64)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_hand_derived_rows(case):
    at, rows = ps.select(vec(case["S"]), vec(case["C"]), vec(case["U"]), case["win_size"], case["min_reads"], bool(case["norm"]), case["p_ratio"])
    assert at.dtype == np.int64 and rows.dtype == np.int64 and rows.shape == (len(at), 3)
    assert at.tolist() == case["ordinals"]
    assert rows.tolist() == case["rows"]
    assert len(case["why"]) >= 1


def test_the_manifest_holds_the_cases_the_rule_turns_on():
    def some(pred):
        return any(pred(c) for c in CASES)
    assert some(lambda c: c["norm"] and c["p_ratio"] < 1.0 and 16777217 in c["C"])          # 2^24 + 1 rounds before the multiply
    assert some(lambda c: c["norm"] and c["p_ratio"] > 1.0 and 16777217 in c["S"])
    assert some(lambda c: c["U"] is not None and c["min_reads"] == 0 and 0 in c["U"])
    assert some(lambda c: c["U"] is not None and any(s > u for s, u in zip(c["S"], c["U"])))
    assert some(lambda c: any(2**31 < v < 2**63 for v in c["S"]))
    assert some(lambda c: c["ordinals"] == [])


def test_float_rounding_is_what_separates_the_rule_from_exact_arithmetic():
    s = np.array([16777217, 16777219], dtype=np.uint64)
    rows = ps.rows_of(s, s, None, 2**40, True, 0.5)
    assert rows[:, 1].tolist() == [8388608, 8388610] and (16777219 * 5) // 10 == 8388609
    rows = ps.rows_of(s, s, None, 2**40, True, 1.0)
    assert rows[:, 0].tolist() == [16777216, 16777220] and rows[:, 1].tolist() == [16777217, 16777219]


def test_no_windows():
    at, rows = ps.select(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), None, 500, 10)
    assert len(at) == 0 and rows.shape == (0, 3)
