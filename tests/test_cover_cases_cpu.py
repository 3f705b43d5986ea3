"""tests/cover_cases.py without a GPU: the pinned kernel constants read back out of the sources, every family's aim (its generator's own
assertions), and the references against each other -- brute() against brute_py() on the small cases and on hand-derived vectors
(tests/golden/cover_cases_manifest.json), brute() against the oracle's two restated algorithms on every case."""
import json
import os
import re

import numpy as np
import pytest

import cover_cases as cc
import switch_points as sp
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
SORTED_FAMILIES = "ABDEG"          # regions in (class, start) order and reads in (class, start) order: the sorted merge takes them too


@pytest.mark.parametrize("name", sorted(cc.SRC))
def test_constant_matches_the_source(name):
    path, pattern, want = cc.SRC[name]
    with open(os.path.join(CSRC, path)) as f:
        found = re.findall(pattern, f.read())
    hint = "%s moved in %s: re-aim the families of tests/cover_cases.py that use it, then update its table" % (name, path)
    assert found, hint + " (no match)"
    for got in found:
        got = got if isinstance(got, tuple) else ((got,) if want else ())
        assert tuple(int(x) for x in got) == tuple(want), hint


def test_minimum_span_by_the_route_rule():
    assert sp.route_answers([q for q, _ in cc.ROUTE_MIN_CPW], {}) == [a for _, a in cc.ROUTE_MIN_CPW]


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_family_aims_and_size_cap(fam):
    cases = cc.family(fam)                      # (the generator's closing assertions ran)
    assert cases
    for v in cc.VARIANTS:
        for c in cc.cases(fam, v)[:3]:
            assert (c.weights is None) == (v == "none") and (c.weights is None or len(c.weights) == len(c.reads))
    w = cc.weights_for("x", 100, "signed")
    assert w.min() == cc.INT32_MIN and w.max() == cc.INT32_MAX


def test_hand_derived_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "cover_cases_manifest.json")) as f:
        man = json.load(f)["cases"]
    assert len(man) >= 12
    for c in man:
        refs, reads = np.array(c["refs"], dtype=np.int32), np.array(c["reads"], dtype=np.int32)
        w = None if c["weights"] is None else np.array(c["weights"], dtype=np.int32)
        want = np.array(c["want"], dtype=np.uint64)
        np.testing.assert_array_equal(cc.brute_py(refs, reads, w), want, err_msg=c["name"])
        np.testing.assert_array_equal(cc.brute(refs, reads, w), want, err_msg=c["name"])


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_brute_equals_python_integers_on_small_cases(fam):
    want = cc.wanted(fam)
    small = [c for c in cc.family(fam) if len(c.reads) <= 300]
    if fam in "ACD":
        assert small
    for c in small:
        got = cc.brute_py_multi(c.refs, c.reads, [cc.weights_for(c.name, len(c.reads), v) for v in cc.VARIANTS])
        for v, g in zip(cc.VARIANTS, got):
            np.testing.assert_array_equal(want[c.name][v], g, err_msg="%s/%s" % (c.name, v))


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_brute_equals_the_oracle(fam):
    want = cc.wanted(fam)
    kept = total = 0
    for c in cc.family(fam):
        take = cc.oracle_takes(c)
        kept, total = kept + int(take.sum()), total + len(take)
        assert fam in "FI" or take.all(), c.name
        reads = c.reads[take]
        algos = [orc.BIN_INDEX]
        if fam in SORTED_FAMILIES and in_order(c.refs) and in_order(reads):
            algos.append(orc.SORTED_MERGE)
        for v in cc.VARIANTS:
            w = cc.weights_for(c.name, len(c.reads), v)
            for algo in algos:
                got = orc.coverage(c.refs, reads, None if w is None else w[take], algo=algo)
                np.testing.assert_array_equal(got, want[c.name][v], err_msg="%s/%s algo %d" % (c.name, v, algo))
    assert kept >= 0.9 * total


def in_order(rows):
    r = np.asarray(rows, dtype=np.int64)
    key = r[:, 0] * (1 << 33) + (r[:, 1] + (1 << 31))
    return bool((np.diff(key) >= 0).all())


def test_the_sorted_merge_ran_somewhere():
    for fam in SORTED_FAMILIES:
        assert any(in_order(c.refs) and in_order(c.reads) for c in cc.family(fam)), fam
