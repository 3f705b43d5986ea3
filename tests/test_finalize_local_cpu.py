"""The two-launch finalize of a large count call (finalize_local_kernel + gather_hits_local_kernel), its threshold and its routing
rule read back out of the sources (no GPU), in the manner of tests/test_switch_points_cpu.py: when one of them moves, this fails
and the cases of tests/test_gpu_finalize_local.py must be re-aimed.

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

LOCAL_SCAN_MAX_TILES = 2048     # local scan + gather up to this many tiles (above CHAIN_MAX_TILES, tile sums not kept)

SRC = {
    "LOCAL_SCAN_MAX_TILES": ("gtx_kernels.h", r"constexpr int kLocalScanMaxTiles = (\d+);", (LOCAL_SCAN_MAX_TILES,)),
    "LOCAL_RULE": ("gtx_kernels.hip", r"if \(!tileSumsValid && totals && totalsTurn && nb <= localMaxTiles\) \{", ()),
    "LOCAL_CLAMP": ("gtx_kernels.hip", r"if \(localMaxTiles > kLocalScanMaxTiles\) localMaxTiles = kLocalScanMaxTiles;", ()),
    "LOCAL_DEFAULT": ("gtx_capi.hip", r"int localMaxTiles = gtx::kLocalScanMaxTiles;", ()),
    "LOCAL_KNOB": ("gtx_capi.hip", r'getenv\("GTX_LOCAL_SCAN_MAX_TILES"\)\) c->localMaxTiles = std::min\(std::max\(atoi\(lt\), 0\), gtx::kLocalScanMaxTiles\);', ()),
    "LOCAL_LDS": ("gtx_kernels.hip", r"kGatherLocalThreads, sizeof\(T\) \* 2 \* \(size_t\)nb, st>>>", ()),
    # the three-launch form it replaces stays, word for word, behind the rule
    "OLD_TILE_SUMS": ("gtx_kernels.hip", r"if \(!tileSumsValid\) tile_sums_kernel<T><<<dim3\(nbRun, 2\), 256, 0, st>>>\(histA, histB, histLen, tileA, tileB, tl\);", ()),
    "OLD_SCAN": ("gtx_kernels.hip", r"finalize_scan_kernel<T><<<dim3\(nbRun, 2\), 256, 0, st>>>\(histA, histB, histLen, tileA, tileB, prefA, prefB, tl\);", ()),
    "OLD_GATHER": ("gtx_kernels.hip", r"gather_hits_kernel<T><<<\(unsigned\)\(\(work \+ 255\) / 256\), 256, 0, st>>>\(prefA, prefB, posE, posS, classBase, mm, hits, tileA, tileB, nb, nextInfo,", ()),
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


@pytest.mark.parametrize("name", ["TILE_SHIFT", "CHAIN_MAX_TILES", "CHAIN_RULE", "TILE_SUMS_MAX_READS"])
def test_older_pinned_lines_are_still_there(name):
    path, pattern, want = sp.SRC[name]
    assert len(re.findall(pattern, source(path))) == 1, name


def test_the_local_rule_sits_in_the_else_branch_of_the_chain_rule():
    text = source("gtx_kernels.hip")
    chain = re.search(sp.SRC["CHAIN_RULE"][1], text).start()
    local = re.search(SRC["LOCAL_RULE"][1], text).start()
    old = re.search(SRC["OLD_TILE_SUMS"][1], text).start()
    assert chain < local < old
    assert re.search(r"\*chainDraws \+= \(unsigned long long\)nbRun;\s*\}\s*else \{\s*" + SRC["LOCAL_RULE"][1], text)


def test_threshold_arithmetic():
    assert sp.CHAIN_MAX_TILES < LOCAL_SCAN_MAX_TILES
    assert sp.tiles(LOCAL_SCAN_MAX_TILES * sp.TILE - 24, 24) == LOCAL_SCAN_MAX_TILES
    assert sp.tiles(LOCAL_SCAN_MAX_TILES * sp.TILE - 23, 24) == LOCAL_SCAN_MAX_TILES + 1
    assert sp.tiles(1_000_000, 24) == 977 and sp.tiles(2_000_000, 24) == 1954          # the two BASELINE shapes are inside
    assert 2 * LOCAL_SCAN_MAX_TILES * 8 == 32 * 1024                                    # the gather's LDS with 64-bit slots
