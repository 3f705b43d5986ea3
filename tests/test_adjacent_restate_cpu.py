"""CPU suite: the Python restatement of `genomic_regions test | gdist | inv` (tests/adjacent_restate.py) against hand-derived vectors
(tests/golden/adjacent_manifest.json, each marked `derived` with the reference lines it follows), and the loops on text against the
loops on packed triples -- the form the C ABI is held to -- on random sets."""
import json
import os

import numpy as np
import pytest

import adjacent_restate as ar

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "adjacent_manifest.json")))
NAMES = ["chr1", "chr10", "chr2", "chrX"]                                        # in strcmp order: the class is 2 * rank + strand


def run_case(case):
    if case["op"] == "inv":
        return ar.inv_lines(case["lines"], case["bounds"])
    if case["op"] == "gdist":
        return ar.gdist_lines(case["lines"], case["op1"], case["op2"])
    return ar.test_lines(case["lines"], case["s"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_hand_derived_output(case):
    assert case["derived"]
    assert run_case(case) == (case["stdout"], case["stderr"], case["code"])


def test_manifest_covers_what_the_issue_lists():
    names = " ".join(c["name"] for c in CASES)
    for word in ("inv_example", "one_base_tail", "start_1_no_leading", "adjacent_and_nested", "two_runs", "strand_change_inside", "missing_chromosome_first",
                 "missing_chromosome_middle", "missing_chromosome_last", "inv_order_error", "inv_multi_interval", "gdist_multi_interval", "nan_across",
                 "unknown_operation", "test_inclusion_overlap_equal_stops", "with_s", "without_s", "test_order_error", "bed12_line_passes",
                 "bed12_line_with_overlapping", "empty_file", "header_lines"):
        assert word in names, word
    assert sum(c["name"].startswith("gdist_minus_pair") for c in CASES) == 16


def random_lines(rng, n, span, by_strand=True, lmax=60):
    """n sorted BED6 lines over NAMES (by chromosome, strand when by_strand, start), with scores, and the same rows as columns"""
    chrom, minus = rng.integers(0, len(NAMES), size=n), rng.integers(0, 2, size=n)
    start = rng.integers(0, span, size=n)
    stop = start + rng.integers(1, lmax, size=n)
    order = np.lexsort((start, minus, chrom)) if by_strand else np.lexsort((start, chrom))
    chrom, minus, start, stop = chrom[order], minus[order], start[order], stop[order]
    score = rng.integers(0, 1000, size=n)
    lines = ["%s\t%d\t%d\tr%d\t%d\t%s" % (NAMES[chrom[k]], start[k], stop[k], k, score[k], "+-"[minus[k]]) for k in range(n)]
    return lines, chrom, minus, start + 1, stop, score


def test_packed_test_loop_agrees_with_the_text_loop():
    rng = np.random.default_rng(21)
    for trial in range(60):
        s = bool(trial & 1)
        lines, chrom, minus, start, stop, _ = random_lines(rng, int(rng.integers(1, 200)), int(rng.choice([300, 5000])), s)
        tri = np.stack([2 * chrom + minus if s else chrom, start, stop], axis=1)
        _, u, n_in, n_ov = ar.adjacent_packed(tri)
        assert u == -1
        assert ar.test_lines(lines, s) == ("", "* The file is sorted! Found %d inclusions and %d overlaps.\n" % (n_in, n_ov), 0)
    assert n_in > 0 and n_ov > 0


def test_packed_test_loop_finds_the_first_unsorted_line():
    rng = np.random.default_rng(22)
    lines, chrom, minus, start, stop, _ = random_lines(rng, 300, 100000, False)
    tri = np.stack([chrom, start, stop], axis=1)
    k = int(np.flatnonzero((chrom[1:] == chrom[:-1]) & (start[1:] > start[:-1]))[40])
    lines[k], lines[k + 1] = lines[k + 1], lines[k]
    tri[[k, k + 1]] = tri[[k + 1, k]]
    _, u, _, _ = ar.adjacent_packed(tri)
    assert u == k + 1
    assert ar.test_lines(lines, False) == ("", "\nError: Line %d: input regions are not sorted (sorted-by-strand = false)!\n" % (k + 2), 1)


def test_packed_distances_agree_with_the_text_loop():
    rng = np.random.default_rng(23)
    for trial in range(64):
        o1, o2 = list(ar.POINTS)[trial % 4], list(ar.POINTS)[(trial // 4) % 4]
        lines, chrom, minus, start, stop, _ = random_lines(rng, int(rng.integers(2, 120)), 2000)
        tri = np.stack([2 * chrom + minus, start, stop], axis=1)
        dist, u, _, _ = ar.adjacent_packed(tri, minus, ar.POINTS[o1], ar.POINTS[o2])
        assert u == -1 and dist[0] == ar.NO_DISTANCE
        want = "".join("r%d\tr%d\t%s\n" % (k - 1, k, "NaN" if dist[k] == ar.NO_DISTANCE else str(int(dist[k]))) for k in range(1, len(lines)))
        assert ar.gdist_lines(lines, o1, o2) == (want, "", 0)


def render_gaps(owners, starts, stops, chrom, minus, score):
    return "".join("%s\t%d\t%d\t_\t%d\t%s\n" % (NAMES[chrom[o]], a - 1, b, score[o], "+-"[minus[o]]) for o, a, b in zip(owners.tolist(), starts.tolist(), stops.tolist()))


def test_packed_gaps_agree_with_the_text_loop():
    rng = np.random.default_rng(24)
    n_gaps = 0
    for trial in range(60):
        span = int(rng.choice([200, 3000]))
        lines, chrom, minus, start, stop, score = random_lines(rng, int(rng.integers(1, 150)), span)
        sizes = {NAMES[k]: int(rng.integers(span - 30, span + 80)) for k in range(len(NAMES))}
        tri = np.stack([2 * chrom + minus, start, stop], axis=1)
        bounds = [sizes[NAMES[k // 2]] for k in range(2 * len(NAMES))]
        owners, starts, stops, bad, kind = ar.gaps_packed(tri, bounds)
        assert (bad, kind) == (-1, 0)
        assert ar.inv_lines(lines, sizes) == (render_gaps(owners, starts, stops, chrom, minus, score), "", 0)
        n_gaps += len(owners)
    assert n_gaps > 500


def test_packed_gaps_stop_where_the_text_loop_stops():
    rng = np.random.default_rng(25)
    lines, chrom, minus, start, stop, score = random_lines(rng, 400, 100000)
    tri = np.stack([2 * chrom + minus, start, stop], axis=1)
    sizes = {c: 200000 for c in NAMES}
    # a missing bound: chr2 (rank 2) is not in the genome file; its first run's head is the first bad row
    part = {c: v for c, v in sizes.items() if c != "chr2"}
    bounds = [part.get(NAMES[k // 2], -1) for k in range(2 * len(NAMES))]
    owners, starts, stops, bad, kind = ar.gaps_packed(tri, bounds)
    assert kind == 2 and bad == int(np.flatnonzero(chrom == 2)[0])
    assert ar.inv_lines(lines, part) == (render_gaps(owners, starts, stops, chrom, minus, score), "Line %d: chromosome chr2 not found!\n" % (bad + 2), 1)
    # an order error inside a run
    same = np.flatnonzero((tri[1:, 0] == tri[:-1, 0]) & (start[1:] > start[:-1]))
    k = int(same[len(same) // 2])
    lines[k], lines[k + 1] = lines[k + 1], lines[k]
    tri[[k, k + 1]] = tri[[k + 1, k]]
    chrom[[k, k + 1]], minus[[k, k + 1]], score[[k, k + 1]] = chrom[[k + 1, k]], minus[[k + 1, k]], score[[k + 1, k]]
    bounds = [sizes[NAMES[j // 2]] for j in range(2 * len(NAMES))]
    owners, starts, stops, bad, kind = ar.gaps_packed(tri, bounds)
    assert (bad, kind) == (k + 1, 1) and len(owners) > 20 and owners.max() <= k
    assert ar.inv_lines(lines, sizes) == (render_gaps(owners, starts, stops, chrom, minus, score),
                                          "\nError: Line %d: input regions are not sorted (sorted-by-strand = true)!\n" % (k + 2), 1)
