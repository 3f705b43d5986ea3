"""tests/scan_cases.py without a GPU: the pinned kernel constants read back out of the sources, every family's aim (its generator's own
assertions), the references against each other -- brute() against brute_py() and against the oracle's unsorted scanner on every case and
weight variant, brute(sorted_rule=True) against the oracle's sorted scanner where that one is defined (reads in order, preprocess '1') --,
the reciprocal estimate scan_slot divides with, and the route rules (tests/switch_points.py, `gtx_packtool route`) for the shapes of the
partition families."""
import os
import re

import numpy as np
import pytest

import scan_cases as sc
import switch_points as sp
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
ALL = sc.FAMILIES + sc.CHILD
N_CASES = {"A": 41, "B": 22, "C": 70, "D": 48, "E": 15, "F": 17, "G": 50, "H": 45}


@pytest.mark.parametrize("name", sorted(sc.SRC))
def test_constant_matches_the_source(name):
    path, pattern, want = sc.SRC[name]
    with open(os.path.join(CSRC, path)) as f:
        found = re.findall(pattern, f.read())
    hint = "%s moved in %s: re-aim the families of tests/scan_cases.py that use it, then update its table" % (name, path)
    assert len(found) == 1, hint + " (%d matches)" % len(found)
    got = found[0] if isinstance(found[0], tuple) else ((found[0],) if want else ())
    assert tuple(int(x) for x in got) == tuple(want), hint


def test_bucket_minimum_is_the_switch_points_one():
    assert sc.BKT_MIN_PER == sp.SCAN_BKT_MIN_PER


@pytest.mark.parametrize("fam", ALL)
def test_family_aims_and_size_cap(fam):
    cases = sc.family(fam)                      # (the generator's closing assertions ran)
    assert len(cases) == N_CASES[fam]
    for c in cases:
        assert c.aim and c.reads.dtype == np.int32 and c.prep in "1c"
        for v in sc.VARIANTS:
            w = sc.weights_for(c.name, len(c.reads), v)
            assert (w is None) == (v == "none") and (w is None or len(w) == len(c.reads))
    w = sc.weights_for("x", 100, "signed")
    assert w.min() == sc.INT32_MIN and w.max() == sc.INT32_MAX


def test_every_listed_seam_has_a_named_case():
    names = {c.name for fam in ALL for c in sc.family(fam)}
    for n in sc.A_SIZES:
        assert "A-n%d" % n in names
    for comb in sc.C_COMB:
        for nw in sc.C_NWIN:
            assert "C-comb%d-nwin%d" % (comb, nw) in names
    for step in sc.B_STEPS:
        assert "B-step%d" % step in names and "B-step%d-centre" % step in names
    for t in (64, 2048):
        assert "E-blocks-T%d-comb1" % t in names and "E-empty-block-T%d" % t in names
    assert {"E-comb2048", "E-comb2049", "E-top-T256", "E-blocks-T128-comb64"} <= names
    for comb in sc.G_COMB:
        for base in sc.G_BASES:
            for n in sc.g_n_micro(base, comb):
                assert any(x.endswith("-comb%d-n%d" % (comb, n)) for x in names if x[0] == "G")


@pytest.mark.parametrize("fam", ALL)
def test_brute_equals_python_integers(fam):
    for rule in (False, True):
        want = sc.wanted(fam, rule)
        for c in sc.family(fam):
            got = sc.brute_py_multi(c.reads, c.class_len, c.step, c.size, c.prep, [sc.weights_for(c.name, len(c.reads), v) for v in sc.VARIANTS], rule)
            for v, g in zip(sc.VARIANTS, got):
                np.testing.assert_array_equal(want[c.name][v], g, err_msg="%s/%s rule %d" % (c.name, v, rule))


def test_brute_on_hand_derived_vectors():
    # two classes, step 2, windows of two steps: positions 1..2 | 3..4 | 5..6 ; the second class has one micro-window and no window
    reads = np.array([[0, 1, 1], [0, 2, 9], [0, 3, 3], [0, 6, 6], [0, 7, 7], [0, 0, 5], [0, 4, 3], [1, 1, 1], [2, 1, 1], [-1, 1, 1]], dtype=np.int32)
    w = np.array([1, 10, 100, 1000, 5, 7, 9, 11, 13, 17], dtype=np.int32)
    for f in (sc.brute, sc.brute_py):
        assert f(reads, (7, 3), 2, 4).tolist() == [3, 2]
        assert f(reads, (7, 3), 2, 4, weights=w).tolist() == [111, 1100]
        assert f(reads, (7, 3), 2, 4, weights=w, sorted_rule=True).tolist() == [127, 1109]       # start 0 becomes 1, the inverted read counts at 4
        assert f(reads, (7, 3), 2, 4, "c", w).tolist() == [108, 1110]                                # centres 1, 5, 3, 6, (7), 2
        assert f(reads, (7, 3), 2, 2, weights=-w).tolist() == [2 ** 64 - 11, 2 ** 64 - 100, 2 ** 64 - 1000, 2 ** 64 - 11]


def oracle_scan(c, w, algo):
    take = sc.oracle_takes(c)
    got, _ = orc.scan(c.reads[take], c.class_len, c.step, c.size, c.prep, None if w is None else w[take], algo=algo)
    return got


@pytest.mark.parametrize("fam", ALL)
def test_brute_equals_the_oracles_unsorted_scanner(fam):
    want = sc.wanted(fam)
    kept = total = 0
    for c in sc.family(fam):
        take = sc.oracle_takes(c)
        kept, total = kept + int(take.sum()), total + len(take)
        for v in sc.VARIANTS:
            got = oracle_scan(c, sc.weights_for(c.name, len(c.reads), v), 0)
            np.testing.assert_array_equal(got, want[c.name][v], err_msg="%s/%s" % (c.name, v))
    assert kept >= 0.97 * total


SORTED_AT_LEAST = {"A": 19, "B": 11, "C": 70, "D": 40, "E": 15, "F": 1, "G": 46, "H": 45}


@pytest.mark.parametrize("fam", ALL)
def test_brute_equals_the_oracles_sorted_scanner(fam):
    want = sc.wanted(fam, True)
    ran = 0
    for c in sc.family(fam):
        if c.prep != "1" or not sc.in_order(c.reads[sc.oracle_takes(c)]):
            continue
        ran += 1
        for v in sc.VARIANTS:
            got = oracle_scan(c, sc.weights_for(c.name, len(c.reads), v), 1)
            np.testing.assert_array_equal(got, want[c.name][v], err_msg="%s/%s" % (c.name, v))
    assert ran >= SORTED_AT_LEAST[fam]


def test_reciprocal_estimate_is_at_most_one_low():
    worst = 0
    for step in sc.B_STEPS:
        xs = set()
        for c in sc.family("B"):
            if c.step == step:
                ok, pos = sc.positions(c.reads, c.prep, True)
                xs |= set((pos[ok] - 1).tolist())
        xs |= {0, 1, step - 1, step, step + 1, sc.TOP - 1, (sc.TOP - 1) // step * step - 1, (sc.TOP - 1) // step * step} - {-1}
        assert max(xs) == sc.TOP - 1 and min(xs) == 0
        lo, hi = sc.reciprocal_worst(step, sorted(xs))
        assert lo >= 0 and hi <= 1, step
        worst = max(worst, hi)
    assert worst == 1                                                                # (the second fix-up has something to do)


def part_cuts(n_micro, per, bins):
    """the edges between the parts of a class of n_micro micro-windows: buckets of `per`, counted in parts of `bins`"""
    return sorted({min(m, n_micro) for f in range(0, n_micro, per) for m in range(f, min(f + per, n_micro) + 1, bins)} | {n_micro})


def test_partition_families_by_the_route_rules():
    """every G and H shape takes the partition path on a context with GTX_BUCKET_MIN_READS=1, its buckets and parts are cut where the
    case says, a window spans a part and a shorter one somewhere, and the parts write the windows themselves up to comb 64 only"""
    assert sp.route_answers(["scan_fused 64 %d 1" % sc.FUSED_MAX_COMB, "scan_fused 65 %d 1" % sc.FUSED_MAX_COMB], {}) == ["1", "0"]
    assert sp.route_answers(["scan_fused 64 %d 1" % sc.FUSED_MAX_COMB], {"GTX_SCAN_FUSED": "0"}) == ["0"]
    short_last = multi = 0
    for fam, env in (("G", {}), ("H", {"GTX_SCAN_BUCKETS": "1"})):
        for c in sc.family(fam):
            total, comb = int(sc.layout(c.class_len, c.step, c.size)[0].sum()), c.size // c.step
            q = ["partition_worth %d 1" % len(c.reads), "scan_per %d %d" % (total, sc.BINS32), "scan_per %d %d" % (total, sc.BINS64),
                 "scan_fused %d %d 1" % (comb, sc.FUSED_MAX_COMB), "scan_tables_ok %d %d %d" % (-(-total // sc.BINS64) + 3, len(c.class_len), total)]
            worth, per32, per64, fused, ok = sp.route_answers(q, env)
            assert worth == "1" and ok == "1" and fused == ("1" if comb <= 64 else "0"), c.name
            n = int(c.class_len[0])
            if fam == "G":
                assert (int(per32), int(per64)) == (sc.BKT_MIN_PER, sc.BINS64), c.name
            else:
                assert (int(per32), int(per64)) == (sc.h_per(n, False), sc.h_per(n, True)), c.name
            for per, bins in ((int(per32), sc.BINS32), (int(per64), sc.BINS64)):
                cuts = part_cuts(n, per, bins)
                sc.g_aim(c, cuts[1:-1], comb)                                         # reads with distinct counts within comb of every cut
                multi += per > bins
                short_last += 0 < cuts[-1] - cuts[-2] < comb - 1
    assert multi >= len(sc.family("H")) and short_last >= 8          # (every H case has a bucket of two or three parts in the kind of call it aims at)


def test_owner_tiles_the_cases_are_built_for():
    assert [sc.own_tile(cap, comb) for cap in (64, None) for comb in (1, 5, 64, 65, 2048, 2049)] == [64, 64, 128, 256, 4096, 0, 2048, 2048, 2048, 2048, 4096, 0]
    for c in sc.family("E") + sc.family("F"):
        take = sc.oracle_takes(c)
        assert not sc.in_order(c.reads) or sc.own_bounds(c.reads, c.class_len, c.step, c.size, 64)[1] == len(c.reads)
        assert take.sum() >= 0.97 * len(take) or c.name[0] == "F"
