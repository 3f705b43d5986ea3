"""The thresholds of tests/switch_points.py: the constants read back out of the sources, the rules asked of the library's own route
functions (csrc/gtx_routes.h, through the host-only `gtx_packtool route`) on both sides of each threshold (no GPU): when one moves,
this fails and names the GPU test of tests/test_gpu_switch_points.py whose cases must be re-aimed.  And the property that keeps the
signal bins' n_dropped at 0."""
import os
import re
import subprocess

import numpy as np
import pytest

import switch_points as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRS = [os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc"), os.path.join(ROOT, "include")]


def source(name):
    for d in DIRS:
        p = os.path.join(d, name)
        if os.path.exists(p):
            with open(p) as f:
                return f.read()
    raise FileNotFoundError(name)


@pytest.mark.parametrize("name", sorted(sp.SRC))
def test_threshold_matches_the_source(name):
    path, pattern, want = sp.SRC[name]
    found = re.findall(pattern, source(path))
    hint = "%s moved in %s: re-aim tests/test_gpu_switch_points.py::%s, then update tests/switch_points.py" % (name, path, sp.AIMED_BY[name])
    assert len(found) == 1, hint + " (pattern matched %d times)" % len(found)
    got = found[0] if isinstance(found[0], tuple) else ((found[0],) if want else ())
    assert tuple(int(x) for x in got) == tuple(want), hint


@pytest.mark.parametrize("name", sorted(sp.ROUTES))
def test_route_rule_at_its_thresholds(name):
    hint = "%s moved in gtx_routes.h: re-aim tests/test_gpu_switch_points.py::%s, then update tests/switch_points.py" % (name, sp.AIMED_BY[name])
    for env in sorted({tuple(e.items()) for e, _, _ in sp.ROUTES[name]}):
        asked = [(q, want) for e, q, want in sp.ROUTES[name] if tuple(e.items()) == env]
        got = sp.route_answers([q for q, _ in asked], dict(env))
        assert got == [want for _, want in asked], hint + " (%s: %s)" % (dict(env), [(q, w, g) for (q, w), g in zip(asked, got) if w != g])


def test_route_knobs_are_read_from_the_environment_only():
    """a knob of the caller's own environment does not leak into a query that names none, and a bad query is refused"""
    os.environ["GTX_CHAIN_MAX_TILES"] = "10"
    try:
        assert sp.route_answers([sp.fin(sp.C, sp.C)], {}) == ["chained"]
    finally:
        del os.environ["GTX_CHAIN_MAX_TILES"]
    assert subprocess.run([sp.PACKTOOL, "route", "finalize", "1"], capture_output=True).returncode == 2
    assert subprocess.run([sp.PACKTOOL, "route", "finalize", "512", "512", "0", "1", "1", "2048"], capture_output=True, text=True).stdout == "chained\n"


def test_every_entry_names_its_gpu_test():
    assert set(sp.AIMED_BY) == set(sp.SRC) | set(sp.ROUTES) and not set(sp.SRC) & set(sp.ROUTES)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_switch_points.py")) as f:
        text = f.read()
    for t in set(sp.AIMED_BY.values()):
        assert re.search(r"^def %s\(" % t, text, re.M), t


def test_table_arithmetic():
    assert sp.TILE == 1 << sp.TILE_SHIFT
    assert sp.tiles(1000, 24) == 1 and sp.tiles(1001, 24) == 2
    assert sp.tiles(sp.CHAIN_MAX_TILES * sp.TILE - 24, 24) == sp.CHAIN_MAX_TILES
    assert sp.tiles(sp.CHAIN_MAX_TILES * sp.TILE - 23, 24) == sp.CHAIN_MAX_TILES + 1
    n1 = sp.JOIN_SCAN_THREADS * sp.JOIN_SCAN_TILE - 1                      # n + 1 offsets fill exactly one partial per lane
    assert sp.join_scan_per(n1) == 1 and sp.join_scan_per(n1 + 1) == 2


def test_signal_bin_never_reaches_n_bins_below_one():
    """bin = (int)(n_bins * z) for 0 <= z < 1 in IEEE doubles: the largest z below 1 is 1 - 2^-53, and for an integer
    n_bins < 2^53 the correctly rounded product n_bins * (1 - 2^-53) is below n_bins -- so the n_dropped branch of the signal
    kernel (and of oracle/restate.py's signal_bin) is unreachable for every n_bins gtx_set_signal_bins takes (< 2^31)"""
    z_max = np.nextafter(1.0, 0.0)
    assert z_max == 1.0 - 2.0 ** -53
    rng = np.random.default_rng(53)
    n = np.concatenate([np.arange(1, 1 << 22, dtype=np.int64),                                # every n_bins up to 4 M
                        rng.integers(1 << 22, 1 << 31, size=1 << 21, dtype=np.int64),         # and random ones up to 2^31
                        np.array([(1 << k) + d for k in range(22, 32) for d in (-2, -1, 0, 1, 2)], dtype=np.int64)])   # powers of two
    n = n[n < (1 << 31)]
    prod = n.astype(np.float64) * z_max                                    # (the monotone worst case of every z < 1)
    assert (np.floor(prod).astype(np.int64) < n).all()
    z = rng.random(1 << 21)                                                # [0, 1) doubles and a few next to 1
    z[:1000] = np.nextafter(1.0, 0.0) - np.arange(1000) * 2.0 ** -53
    nb = rng.integers(1, 1 << 31, size=z.size, dtype=np.int64)
    assert (np.floor(nb.astype(np.float64) * z).astype(np.int64) < nb).all()
