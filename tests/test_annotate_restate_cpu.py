"""CPU suite: the Python restatement of `genomic_overlaps annotate` and of its upstream builder (tests/annotate_restate.py) against
hand-derived vectors (tests/golden/annotate_manifest.json: each carries its derivation and the reference lines it rests on)."""
import copy
import json
import os

import pytest

import annotate_restate as ar

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "annotate_manifest.json")))
BUILDER, ANNOTATE = MANIFEST["builder"], MANIFEST["annotate"]


def build(case):
    try:
        up = ar.upstream_set(ar.regions_of(case["genes"]), copy.deepcopy(case["bounds"]), case["ignore_strand"], case["upstream_max"], case["upstream_min"])
    except ar.InputError as err:
        return "", err.stderr(), 1
    return ar.reg_lines(up), "", 0


@pytest.mark.parametrize("case", BUILDER, ids=[c["name"] for c in BUILDER])
def test_builder_gives_the_hand_derived_set(case):
    assert case["derived"] and case["derivation"]
    assert build(case) == (case["stdout"], case["stderr"], case["code"])


@pytest.mark.parametrize("case", ANNOTATE, ids=[c["name"] for c in ANNOTATE])
def test_annotate_gives_the_hand_derived_output(case):
    assert case["derived"] and case["derivation"]
    assert ar.annotate(case["genes"], case["tests"], **case["opts"]) == (case["stdout"], case["stderr"], case["code"])


def test_manifest_covers_what_the_issue_lists():
    names = " ".join(c["name"] for c in BUILDER + ANNOTATE)
    for word in ("both_strands", "start_clamp_at_1", "gene_at_start_1", "bound_clamp", "missing_bound", "inverted_region_from_a_clamp", "widen_back",
                 "trimmed_to_nothing", "centre_sums_minus1_0_plus1", "distance_flag_at_exactly_proximal_dist", "minus_strand", "bad_query_op",
                 "bed12_test_line", "multi_interval_reference", "overlaps_its_upstream"):
        assert word in names, word


def test_a_missing_bound_is_inserted_like_operator_brackets():
    bounds = {"chr1": 5000}
    ar.upstream_set(ar.regions_of(["chr7\t99\t200\tg\t0\t-"]), bounds, False, 500, 500)
    assert bounds == {"chr1": 5000, "chr7": 0}


def test_index_order_is_level_bin_then_last_inserted_first():
    """three regions in one level-0 bin come back last first; a region spanning two level-0 bins sits a level up and comes later"""
    regs = ar.regions_of(["chr1\t10\t20\ta", "chr1\t12\t30\tb", "chr1\t0\t200000\twide", "chr1\t15\t18\tc"])
    key = ar.index_order(regs)
    assert ar.overlaps_in_order(regs, key, "chr1", "+", 16, 17, False) == [3, 1, 0, 2]
