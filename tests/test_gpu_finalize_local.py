"""The two-launch finalize of a large count call -- finalize_local_kernel (tile-local prefixes + the tiles' totals) and
gather_hits_local_kernel (every block scans the totals into LDS for itself and adds the tiles' offsets while it gathers) -- against
the CPU oracle (oracle/orc.py), exact.  It serves a call whose tile sums were not kept (TILE_SUMS_MAX_READS reads or more), above
CHAIN_MAX_TILES tiles and up to LOCAL_SCAN_MAX_TILES tiles (tests/test_finalize_local_cpu.py reads the rule back out of the
sources); GTX_LOCAL_SCAN_MAX_TILES, read when a context is made, moves the limit.  Every case asserts the tile count that decides
its route."""
import ctypes
import os

import numpy as np
import pytest

import gtx
import switch_points as sp
import test_gpu_switch_points as tsp
from oracle import orc
from test_finalize_local_cpu import LOCAL_SCAN_MAX_TILES

pytestmark = pytest.mark.gpu

N_CLASSES = tsp.N_CLASSES
N_READS = sp.TILE_SUMS_MAX_READS                     # the smallest launch that leaves the tile sums to the finalize step


@pytest.fixture(scope="module")
def reads_a():
    rng = np.random.default_rng(3030)
    reads = tsp.class_reads(rng, N_READS)
    return reads, rng.integers(-3, 9, size=len(reads)).astype(np.int32)


@pytest.fixture(scope="module")
def refs513(reads_a):
    """CHAIN_MAX_TILES + 1 tiles over 24 even classes (the chained kernel is out), and the oracle's counts of reads_a"""
    refs = tsp.class_refs(np.random.default_rng(513), tsp.spread(sp.CHAIN_MAX_TILES * sp.TILE - N_CLASSES + 1))
    assert sp.tiles(len(refs), N_CLASSES) == sp.CHAIN_MAX_TILES + 1
    return refs, orc.count(refs, reads_a[0], algo=orc.SORTED_MERGE), orc.count(refs, reads_a[0], reads_a[1], algo=orc.SORTED_MERGE)


def three_entries(e, torch, refs, reads, w, want, want_w):
    """the host entry (64-bit slots), the device entry (32-bit slots), the device entry with weights (64-bit, some negative)"""
    assert len(reads) >= sp.TILE_SUMS_MAX_READS and (w < 0).any()
    hits, info = e.count(reads, None, gtx.READS_SORTED)
    np.testing.assert_array_equal(hits, want)
    assert info["n_no_class"] == 0
    got, _ = tsp.device_counts(e, torch, reads, len(refs))
    np.testing.assert_array_equal(got, want)
    got, _ = tsp.device_counts(e, torch, reads, len(refs), w)
    np.testing.assert_array_equal(got, want_w)


@pytest.mark.parametrize("knob", [sp.CHAIN_MAX_TILES + 1, sp.CHAIN_MAX_TILES], ids=["local", "three_launches"])
def test_both_routes_on_the_same_inputs(reads_a, refs513, knob):
    """513 tiles with the limit at 513 (local scan + gather) and at 512 (tile_sums + finalize_scan + gather_hits)"""
    torch = pytest.importorskip("torch")
    refs, want, want_w = refs513
    assert want[:64].sum() > 0 and want[-64:].sum() > 0 and (want > 0).mean() > 0.9
    e = tsp.engine_with(GTX_LOCAL_SCAN_MAX_TILES=knob)
    try:
        e.set_refs(refs, N_CLASSES)
        three_entries(e, torch, refs, reads_a[0], reads_a[1], want, want_w)
    finally:
        e.close()


def edge_layout():
    """class 1 starts exactly on the first slot of tile 300, class 2 is empty (its one slot: the first of tile 521), 522 tiles, the
    last one partial"""
    per_class = np.array([300 * sp.TILE - 1, 221 * sp.TILE - 1, 0] + [1] * (N_CLASSES - 3))
    first_slot = np.concatenate(([0], np.cumsum(per_class)[:-1])) + np.arange(N_CLASSES)
    assert first_slot[1] == 300 * sp.TILE and first_slot[2] == 521 * sp.TILE and per_class[2] == 0
    n_slots = int(per_class.sum()) + N_CLASSES
    assert sp.tiles(int(per_class.sum()), N_CLASSES) == 522 > sp.CHAIN_MAX_TILES and n_slots % sp.TILE != 0
    return per_class


def test_class_edges_on_tile_edges(engine, reads_a):
    torch = pytest.importorskip("torch")
    refs = tsp.class_refs(np.random.default_rng(522), edge_layout())
    reads, w = reads_a
    want, want_w = orc.count(refs, reads, algo=orc.SORTED_MERGE), orc.count(refs, reads, w, algo=orc.SORTED_MERGE)
    cls = refs[:, 0]
    assert want[cls == 0][-1] > 0 and want[cls == 1][0] > 0 and want[cls == 1][-1] > 0 and want[cls == 3][0] > 0 and want[-1] > 0
    engine.set_refs(refs, N_CLASSES)
    three_entries(engine, torch, refs, reads, w, want, want_w)


def test_repeated_calls_leave_histograms_and_totals_clean(engine, reads_a, refs513):
    """two read sets in turn on one context, five calls: either pair of totals is written twice and must have been left zero"""
    torch = pytest.importorskip("torch")
    refs, want_a, _ = refs513
    reads_b = tsp.class_reads(np.random.default_rng(3131), N_READS + 77)
    want_b = orc.count(refs, reads_b, algo=orc.SORTED_MERGE)
    assert not np.array_equal(want_a, want_b)
    engine.set_refs(refs, N_CLASSES)
    for k in range(5):
        reads, want = (reads_a[0], want_a) if k % 2 == 0 else (reads_b, want_b)
        got, _ = tsp.device_counts(engine, torch, reads, len(refs))
        np.testing.assert_array_equal(got, want, err_msg="call %d" % k)
    hits, _ = engine.count(reads_a[0], None, gtx.READS_SORTED)               # ... and the host entry's 64-bit slots behind them
    np.testing.assert_array_equal(hits, want_a)


@pytest.mark.parametrize("extra", [0, 1], ids=["tiles2048", "tiles2049"])
def test_the_default_limit(engine, reads_a, extra):
    """LOCAL_SCAN_MAX_TILES tiles: local scan + gather with the largest LDS; one tile more: the three launches"""
    torch = pytest.importorskip("torch")
    refs = tsp.class_refs(np.random.default_rng(2048 + extra), tsp.spread(LOCAL_SCAN_MAX_TILES * sp.TILE - N_CLASSES + extra), span=8_000_000)
    assert sp.tiles(len(refs), N_CLASSES) == LOCAL_SCAN_MAX_TILES + extra
    rng = np.random.default_rng(77)
    reads = tsp.class_reads(rng, N_READS, span=8_000_000)
    want = orc.count(refs, reads, algo=orc.SORTED_MERGE)
    assert want[:64].sum() > 0 and want[-64:].sum() > 0
    engine.set_refs(refs, N_CLASSES)
    got, _ = tsp.device_counts(engine, torch, reads, len(refs))
    np.testing.assert_array_equal(got, want)


def listed_tiles(refs, owner, member):
    """the tiles gtxi_set_share lists for a member: those that hold a slot of a class it owns or the slot below the class's first"""
    seg = np.concatenate(([0], np.cumsum(np.bincount(refs[:, 0], minlength=N_CLASSES))))
    mark = set()
    for c in np.nonzero(owner == member)[0]:
        if seg[c] == seg[c + 1]:
            continue
        mark.update(range(max(0, seg[c] + c - 1) >> sp.TILE_SHIFT, ((seg[c + 1] + c) >> sp.TILE_SHIFT) + 1))
    return len(mark)


def next_totals_nonzero(g, member, hist_set):
    """gtxi_next_totals_nonzero: words that are not zero in the tile totals which the next two-launch finalize on a member's
    histogram set (-1: the context's own) will write"""
    n = ctypes.c_int64(-1)
    assert g.lib.gtxi_next_totals_nonzero(ctypes.c_void_p(g.ctx(member)), ctypes.c_int(hist_set), ctypes.byref(n)) == 0
    return n.value


def test_group_members_after_a_new_assignment():
    """A member finalizes the tiles of its classes only, so the totals of the other tiles must read as zero -- also those an earlier
    assignment of the same member wrote.  Each histogram set of a context takes its two pairs of totals in turn, and the gather of a
    call zeroes the pair the next call on the set writes.  The group runs with ONE stream per member (GTX_GROUP_STREAMS=1, read at
    the first device call), so that all sorted calls of a member land on its set 0: calls 1 and 2 (first assignment) write pair 0
    and pair 1, call 3 -- the first after the new assignment -- writes pair 0 again, which call 1 wrote under the FIRST assignment
    and call 2's gather zeroed.  The calls with flags = 0 take the member's own stream and the context's own set: two before the new
    assignment, and the one after it writes the pair the first of them wrote.
    Equal counts alone would not show a pair left dirty: the offsets of tiles outside a member's list enter both ends of every
    difference the gather takes and cancel.  So the state itself is read back after every call (gtxi_next_totals_nonzero): the pair
    about to be written holds no word that is not zero."""
    torch = pytest.importorskip("torch")
    old = os.environ.get("GTX_GROUP_STREAMS")
    os.environ["GTX_GROUP_REHEARSE"] = "1"; os.environ["GTX_GROUP_STREAMS"] = "1"
    g = None
    try:
        g = gtx.Group([0, 0])
        rng = np.random.default_rng(1100)
        refs = tsp.class_refs(rng, tsp.spread(1040 * sp.TILE), span=4_000_000)
        assert sp.CHAIN_MAX_TILES < sp.tiles(len(refs), N_CLASSES) <= LOCAL_SCAN_MAX_TILES
        reads = tsp.class_reads(rng, 2 * N_READS + N_READS // 4, span=4_000_000)
        want = orc.count(refs, reads, algo=orc.SORTED_MERGE)
        assert (want > 0).mean() > 0.9
        g.set_refs(refs, N_CLASSES)
        hits = torch.full((len(refs),), -1, dtype=torch.int64, device="cuda")
        owners = []
        for load, flag_seq in ((np.bincount(reads[:, 0], minlength=N_CLASSES), (gtx.READS_SORTED, gtx.READS_SORTED, 0, 0)),
                               (np.arange(N_CLASSES, 0, -1), (gtx.READS_SORTED, gtx.READS_SORTED, 0))):
            owner = g.assign(load)
            owners.append(owner.copy())
            # either member lists more tiles than the chained kernel takes: both finalize with the local scan + gather
            assert min(listed_tiles(refs, owner, m) for m in range(2)) > sp.CHAIN_MAX_TILES
            own = owner[reads[:, 0]]
            parts = [np.ascontiguousarray(reads[own == m]) for m in range(2)]
            assert min(len(p) for p in parts) >= sp.TILE_SUMS_MAX_READS
            dev = [torch.from_numpy(p).cuda() for p in parts]
            for flags in flag_seq:
                hits.fill_(-1)
                g.count_device([d.data_ptr() for d in dev], [len(p) for p in parts], hits.data_ptr(), flags=flags)
                g.sync()
                np.testing.assert_array_equal(hits.cpu().numpy().view(np.uint64), want)
                for m in range(2):
                    assert next_totals_nonzero(g, m, 0) == 0 and next_totals_nonzero(g, m, -1) == 0
        assert not np.array_equal(owners[0], owners[1])
        # (the sets the one-stream group never took were never made: nothing to read there)
        assert next_totals_nonzero(g, 0, 1) == 0
    finally:
        del os.environ["GTX_GROUP_REHEARSE"]
        if old is None:
            del os.environ["GTX_GROUP_STREAMS"]
        else:
            os.environ["GTX_GROUP_STREAMS"] = old
        if g is not None:
            g.close()
