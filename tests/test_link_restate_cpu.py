"""CPU suite: the Python restatement of `genomic_regions link` (tests/link_restate.py) against hand-derived vectors
(tests/golden/link_manifest.json, each marked `derived` with the reference lines it follows), and the parallel form the device
computes against the sequential loop."""
import json
import os

import numpy as np
import pytest

import link_restate

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "link_manifest.json")))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_hand_derived_output(case):
    assert case["derived"]
    out, err, code = link_restate.link_lines(case["lines"], case["s"], case["d"], case["label_func"])
    assert (out, err, code) == (case["stdout"], case["stderr"], case["code"])


def test_manifest_covers_what_the_issue_lists():
    names = " ".join(c["name"] for c in CASES)
    for word in ("d0_adjacent", "d1_adjacent", "contained", "d_minus5", "zero_length", "without_s", "with_s", "heads_strand", "label_sum", "label_min",
                 "label_max", "label_delimiter", "1e+06", "order_error", "multi_interval_error"):
        assert word in names


def test_packed_loop_agrees_with_the_text_loop():
    lines = ["chr1\t0\t100\t5", "chr1\t10\t20\t7", "chr1\t50\t150\t1", "chr1\t300\t310\t2", "chr2\t0\t5\t9"]
    tri = np.array([[0, 1, 100], [0, 11, 20], [0, 51, 150], [0, 301, 310], [1, 1, 5]])
    h, c, s, v, u = link_restate.link_packed(tri, 0, [5, 7, 1, 2, 9], "sum")
    assert (h.tolist(), c.tolist(), s.tolist(), v.tolist(), u) == ([0, 3, 4], [3, 1, 1], [150, 310, 5], [13, 2, 9], -1)
    out, _, _ = link_restate.link_lines(lines, False, 0, "sum")
    assert out == "13\tchr1 + 1 150\n2\tchr1 + 301 310\n9\tchr2 + 1 5\n"


def test_packed_loop_stops_at_the_first_unsorted_row():
    tri = np.array([[0, 1, 10], [0, 20, 30], [0, 40, 50], [0, 35, 60], [0, 70, 80]])
    h, c, s, _, u = link_restate.link_packed(tri, 0)
    assert (h.tolist(), c.tolist(), s.tolist(), u) == ([0, 1], [1, 1], [10, 30], 3)     # the group open at row 3 is not reported


def parallel_form(tri, d):
    """heads by the class prefix maximum (include/gtx.h); stops as the maximum over each group's own members"""
    n = len(tri)
    head = np.zeros(n, dtype=bool)
    p = None
    for i in range(n):
        if i == 0 or tri[i, 0] != tri[i - 1, 0]:
            head[i] = True; p = int(tri[i, 2])
        else:
            head[i] = int(tri[i, 1]) - p > d
            p = max(p, int(tri[i, 2]))
    at = np.flatnonzero(head)
    stops = [int(tri[a:b, 2].max()) for a, b in zip(at, list(at[1:]) + [n])]
    return at, stops, head


def test_parallel_form_equals_the_loop_and_the_prefix_shortcut_does_not():
    rng = np.random.default_rng(11)
    shortcut_wrong = 0
    for trial in range(600):
        n = int(rng.integers(1, 40))
        cls = np.sort(rng.integers(0, 3, size=n))
        start = rng.integers(0, 60, size=n)
        order = np.lexsort((start, cls))
        cls, start = cls[order], start[order]
        stop = start + rng.integers(-4, 12, size=n) - 1
        tri = np.stack([cls, start, stop], axis=1)
        d = int(rng.choice([0, 1, -1, -5, 7, 100]))
        h, c, s, _, u = link_restate.link_packed(tri, d)
        at, stops, head = parallel_form(tri, d)
        assert u == -1 and h.tolist() == at.tolist() and s.tolist() == stops
        pm = [int(tri[:b][tri[:b, 0] == tri[b - 1, 0]][:, 2].max()) for b in list(at[1:]) + [n]]   # the class prefix maximum at each group's last member
        shortcut_wrong += pm != stops
    assert shortcut_wrong > 0      # the shapes above do catch the shortcut
