"""The two-launch finalize of a large count call (finalize_local_kernel + gather_hits_local_kernel): its threshold read back out of
the sources, its routing rule asked of the library's own finalize_route (csrc/gtx_routes.h through `gtx_packtool route`) on both sides
of every threshold (no GPU), in the manner of tests/test_switch_points_cpu.py: when one of them moves, this fails and the cases of
tests/test_gpu_finalize_local.py must be re-aimed.

The rule: a call whose tile sums were not kept (TILE_SUMS_MAX_READS reads or more in the launch) and that does not take the chained
kernel (more than CHAIN_MAX_TILES tiles, or no chain flags) takes the local scan + gather while the histograms have at most
LOCAL_SCAN_MAX_TILES tiles -- all the tiles, not a group member's listed ones: the gather keeps one offset per tile and histogram
in LDS.  GTX_LOCAL_SCAN_MAX_TILES (read per context in gtx_create, clamped to the default) moves the limit; 0 restores
tile_sums + finalize_scan + gather_hits."""
import os
import re

import pytest

import switch_points as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")

LOCAL_SCAN_MAX_TILES = sp.LOCAL_SCAN_MAX_TILES     # local scan + gather up to this many tiles (above CHAIN_MAX_TILES, tile sums not kept)

SRC = {
    "LOCAL_SCAN_MAX_TILES": ("gtx_routes.h", r"constexpr int kLocalScanMaxTiles = (\d+);", (LOCAL_SCAN_MAX_TILES,)),
    "LOCAL_DEFAULT": ("gtx_ctx.h", r"int localMaxTiles = gtx::kLocalScanMaxTiles;", ()),
    "LOCAL_KNOB": ("gtx_capi.hip", r'getenv\("GTX_LOCAL_SCAN_MAX_TILES"\)\) c->localMaxTiles = std::min\(std::max\(atoi\(lt\), 0\), gtx::kLocalScanMaxTiles\);', ()),
    "LOCAL_LDS": ("gtx_kernels.hip", r"kGatherLocalThreads, sizeof\(T\) \* 2 \* \(size_t\)nb, st>>>", ()),
}

fin, C, L, EVERY_TILE_COUNT, NO_CHAIN = sp.fin, sp.C, sp.L, sp.EVERY_TILE_COUNT, sp.NO_CHAIN
ROUTES = {
    # ... else the local scan + gather up to LOCAL_SCAN_MAX_TILES tiles IN ALL (not the ones run: the gather keeps an offset per tile) ...
    "LOCAL_RULE": [({}, fin(C + 1, C + 1), "local"), ({}, fin(L, L), "local"), ({}, fin(L + 1, L + 1), "sums_scan"), ({}, fin(L, 600), "local"),
                   ({}, fin(3000, 600), "sums_scan"), ({}, fin(L + 1, C + 1), "sums_scan"), ({}, fin(C + 1, C + 1, totals=0), "sums_scan"),
                   ({}, fin(C, C, chain=0, totals=0), "sums_scan"), (NO_CHAIN, fin(C, C, totals=0), "sums_scan")],
    # ... the context's limit clamped to the constant (the gather's LDS), 0 = never
    "LOCAL_CLAMP": [({}, fin(C + 1, C + 1, local_max=C), "sums_scan"), ({}, fin(C + 1, C + 1, local_max=C + 1), "local"),
                    ({}, fin(L, L, local_max=5000), "local"), ({}, fin(L + 1, L + 1, local_max=5000), "sums_scan"),
                    ({}, fin(C + 1, C + 1, local_max=0), "sums_scan"), (NO_CHAIN, fin(1, 1, local_max=0), "sums_scan")],
    # the three-launch form stays behind the two rules: tile sums only when they were not kept, and the plain gather without tiles to run
    "OLD_TILE_SUMS": [({}, fin(L + 1, L + 1), "sums_scan"), ({}, fin(L + 1, L + 1, sums_valid=1), "sums_kept")],
    "OLD_SCAN": [({}, fin(n, n, sums_valid=1), "sums_kept") for n in EVERY_TILE_COUNT] +
                [({}, fin(977, 100, sums_valid=1), "sums_kept"), ({}, fin(3000, 600, sums_valid=1), "sums_kept"), (NO_CHAIN, fin(C, C, sums_valid=1), "sums_kept"),
                 ({}, fin(C, C, sums_valid=1, chain=0, totals=0), "sums_kept")],
    "OLD_GATHER": [({}, fin(977, 0), "gather_only"), ({}, fin(977, 0, sums_valid=1), "gather_only"), ({}, fin(0, 0), "gather_only"),
                   ({}, fin(3000, 0, chain=0, totals=0), "gather_only")],
    # the local rule is asked only where the chain rule said no: a shape both would take is chained
    "LOCAL_AFTER_CHAIN": [({}, fin(C, C), "chained"), ({}, fin(1, 1), "chained"), ({}, fin(L, C), "chained"), ({}, fin(L + 1, C), "chained")],
}


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(SRC))
def test_local_finalize_matches_the_source(name):
    path, pattern, want = SRC[name]
    found = re.findall(pattern, source(path))
    assert len(found) == 1, "%s moved in %s: re-aim tests/test_gpu_finalize_local.py (pattern matched %d times)" % (name, path, len(found))
    assert tuple(int(x) for x in ((found[0],) if want else ())) == tuple(want)


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_local_finalize_route(name):
    for env in ({}, NO_CHAIN):
        asked = [(q, want) for e, q, want in ROUTES[name] if e == env]
        got = sp.route_answers([q for q, _ in asked], env)
        assert got == [want for _, want in asked], "%s moved: re-aim tests/test_gpu_finalize_local.py (%s: %s)" % (name, env, list(zip(asked, got)))
    assert all(e in ({}, NO_CHAIN) for e, _, _ in ROUTES[name])


@pytest.mark.parametrize("name", ["TILE_SHIFT", "CHAIN_MAX_TILES", "TILE_SUMS_MAX_READS"])
def test_older_pinned_lines_are_still_there(name):
    path, pattern, want = sp.SRC[name]
    assert len(re.findall(pattern, source(path))) == 1, name


def test_older_chain_rule_still_holds():
    for env in sorted({tuple(e.items()) for e, _, _ in sp.ROUTES["CHAIN_RULE"]}):
        asked = [(q, want) for e, q, want in sp.ROUTES["CHAIN_RULE"] if tuple(e.items()) == env]
        assert sp.route_answers([q for q, _ in asked], dict(env)) == [want for _, want in asked], env


def test_threshold_arithmetic():
    assert sp.CHAIN_MAX_TILES < LOCAL_SCAN_MAX_TILES
    assert sp.tiles(LOCAL_SCAN_MAX_TILES * sp.TILE - 24, 24) == LOCAL_SCAN_MAX_TILES
    assert sp.tiles(LOCAL_SCAN_MAX_TILES * sp.TILE - 23, 24) == LOCAL_SCAN_MAX_TILES + 1
    assert sp.tiles(1_000_000, 24) == 977 and sp.tiles(2_000_000, 24) == 1954          # the two BASELINE shapes are inside
    assert 2 * LOCAL_SCAN_MAX_TILES * 8 == 32 * 1024                                    # the gather's LDS with 64-bit slots
