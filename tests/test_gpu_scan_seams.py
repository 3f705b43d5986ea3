"""The window scans at every tile, part, window and class seam: the cases of tests/scan_cases.py -- each family aims at one kind of edge and
says so in assertions of its own -- against the brute-force definition scan_cases.brute(), bit for bit, unweighted and with three kinds of
weights, through every route a shape admits: the general kernels (scan_hist_kernel + scan_window_kernel), the owner-computes pass with
blocks of 64 windows and of the default size, its fallback on reads that are not in order, the partition path with the micro-window array
and with the parts writing the windows themselves (bucket_scanhist_kernel with `out`, scan_zero_edges_kernel), streamed calls, and -- for
the knobs a process reads once -- tests/scan_seams_child.py.  tests/test_scan_cases_cpu.py holds the references against each other and
against the oracle, and the kernel constants the cases aim at."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import gtx
import scan_cases as sc
import switch_points as sp

pytestmark = pytest.mark.gpu

DEVICE_VARIANTS = ("none", "signed")
SENTINEL = 0x5A5A5A5A5A5A5A5A            # what the output of a device call holds beforehand: a window nobody writes shows
BENG_MIN_READS = 1
CAPS = (64, None)                        # GTX_SCAN_OWN_TILE
RULES = ((False, 0), (True, gtx.ZERO_LENGTH_OK))


def make_engine(**env):
    os.environ.update(env)
    try:
        return gtx.Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def beng():
    e = make_engine(GTX_BUCKET_MIN_READS=str(BENG_MIN_READS))
    yield e
    e.close()


@contextlib.contextmanager
def owner_knobs(cap):
    """GTX_SCAN_OWN_ALWAYS and GTX_SCAN_OWN_TILE are read at every call"""
    keep = {k: os.environ.get(k) for k in ("GTX_SCAN_OWN_ALWAYS", "GTX_SCAN_OWN_TILE")}
    os.environ["GTX_SCAN_OWN_ALWAYS"] = "1"
    os.environ.pop("GTX_SCAN_OWN_TILE", None)
    if cap is not None:
        os.environ["GTX_SCAN_OWN_TILE"] = str(cap)
    try:
        yield
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def host_scan(e, c, reads, w, flags):
    got, _ = e.scan(reads, c.class_len, c.step, c.size, c.prep, weights=w, flags=flags)
    return got


def device_scan(e, c, reads, w, flags):
    import torch
    dev = torch.device("cuda", 0)
    tot = sc.layout(c.class_len, c.step, c.size)[3]
    d_reads = torch.from_numpy(np.array(reads, dtype=np.int32)).to(dev)
    d_w = None if w is None else torch.from_numpy(np.array(w, dtype=np.int32)).to(dev)
    d_out = torch.full((max(tot, 1),), SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    e.scan_device(d_reads.data_ptr() if len(reads) else None, len(reads), c.class_len, c.step, c.size, d_out.data_ptr(), c.prep,
                  None if d_w is None or not len(reads) else d_w.data_ptr(), flags)
    e.sync()
    return d_out.cpu().numpy().view(np.uint64)[:tot]


def expect(c, rule):
    return sc.wanted(c.name[0], rule)[c.name]


def run(call, e, c, variants, flags, rule, tag, reads=None, perm=None):
    for v in variants:
        w = sc.weights_for(c.name, len(c.reads), v)
        if w is not None and perm is not None:
            w = np.ascontiguousarray(w[perm])
        got = call(e, c, c.reads if reads is None else reads, w, flags)
        np.testing.assert_array_equal(got, expect(c, rule)[v], err_msg="%s/%s %s" % (c.name, v, tag))


def windows(c):
    return sc.layout(c.class_len, c.step, c.size)[3]


def general(e, c):
    """scan_hist_kernel + scan_window_kernel: no hint, fewer reads than the context's bucket minimum, under both rules"""
    assert len(c.reads) < sp.BUCKET_MIN_READS
    for rule, fl in RULES:
        run(host_scan, e, c, sc.VARIANTS, fl, rule, "general, host, rule %d" % rule)
        run(device_scan, e, c, DEVICE_VARIANTS, fl, rule, "general, device, rule %d" % rule)


def owner(e, c, takes):
    """GTX_READS_SORTED with the pass forced on any geometry, blocks of 64 windows and of the default size, host entry (the reads made
    resident) and device entry, both rules; takes: whether the pass serves (reads in order) or gives up for the general kernels"""
    assert c.prep == "1"
    comb = c.size // c.step
    for cap in CAPS:
        tile = sc.own_tile(cap, comb)
        assert takes == sc.in_order(c.reads) and (tile > 0) == (comb <= sc.WIN_MAX_COMB), c.name
        with owner_knobs(cap):
            for rule, fl in RULES:
                run(host_scan, e, c, sc.VARIANTS, fl | gtx.READS_SORTED, rule, "owner, tile %d, host, rule %d" % (tile, rule))
                run(device_scan, e, c, DEVICE_VARIANTS, fl | gtx.READS_SORTED, rule, "owner, tile %d, device, rule %d" % (tile, rule))


def partition(e, c):
    """a context with a bucket minimum of one read, GTX_READS_UNSORTED, the reads shuffled: the host entry keeps the micro-window array,
    the device entry lets the parts write the windows (comb <= 64) into an output that held the sentinel"""
    reads, perm = sc.shuffled(c)
    takes = BENG_MIN_READS <= len(reads) < 1 << 31
    assert takes == (len(reads) > 0)
    run(host_scan, e, c, sc.VARIANTS, gtx.READS_UNSORTED, False, "partition, host", reads, perm)
    run(device_scan, e, c, sc.VARIANTS, gtx.READS_UNSORTED, False, "partition, device (fused: %d)" % fused(c), reads, perm)
    return takes and fused(c)


def fused(c):
    return c.size // c.step <= sc.FUSED_MAX_COMB and windows(c) > 0


def check_family(fam, engine, beng):
    ran = n_fused = n_owner = 0
    for c in sc.family(fam):
        ran += 1
        general(engine, c)
        if c.prep == "1":
            owner(engine, c, sc.in_order(c.reads))
            n_owner += sc.in_order(c.reads)
        n_fused += partition(beng, c)
    assert ran == len(sc.family(fam))
    return ran, n_owner, n_fused


def test_a_reads_per_step_and_classes_in_a_step(engine, beng):
    assert check_family("A", engine, beng) == (41, 27, 40)                 # (A-n0 has no read to partition)


def test_b_the_division(engine, beng):
    assert check_family("B", engine, beng) == (22, 11, 22)


@pytest.mark.parametrize("comb", sc.C_COMB)
def test_c_window_sums(engine, beng, comb):
    ran = n_fused = 0
    for c in sc.family("C"):
        if c.size // c.step != comb:
            continue
        ran += 1
        general(engine, c)
        owner(engine, c, True)
        n_fused += partition(beng, c)
    assert ran == len(sc.C_NWIN) and n_fused == (ran if comb <= sc.FUSED_MAX_COMB else 0)


def test_d_the_lds_tile_of_the_histogram_pass(engine, beng):
    assert check_family("D", engine, beng) == (48, 42, 48)


def test_e_owner_blocks(engine, beng):
    ran, n_owner, n_fused = check_family("E", engine, beng)
    assert (ran, n_owner, n_fused) == (15, 15, 12)                         # (comb 2048, 2049 and 65 keep the micro-window array)
    assert sc.own_tile(64, 2048) == 4096 and sc.own_tile(None, 2049) == 0


def test_f_the_order_check_of_the_owner_pass(engine, beng):
    base = sc.by_name("F-in-order")
    ran = 0
    for c in sc.family("F"):
        ran += 1
        broken = c is not base
        assert sc.in_order(c.reads) == (not broken)
        owner(engine, c, not broken)
        if broken:                                                         # the flag a broken stream raised is gone: the owner pass serves again
            with owner_knobs(64):
                run(host_scan, engine, base, ("none", "signed"), gtx.READS_SORTED, False, "in order right after %s" % c.name)
                run(device_scan, engine, base, ("none",), gtx.READS_SORTED | gtx.ZERO_LENGTH_OK, True, "in order right after %s, device" % c.name)
        general(engine, c)
        partition(beng, c)
    assert ran == 17


def test_g_parts_and_buckets_of_the_partition_path(engine, beng):
    ran = n_fused = 0
    for c in sc.family("G"):
        ran += 1
        n_fused += partition(beng, c)
        run(host_scan, engine, c, ("none", "signed"), 0, False, "general, host")
        if c.prep == "1":
            with owner_knobs(None):
                run(device_scan, engine, c, ("none",), gtx.READS_SORTED, False, "owner, device")
    assert ran == 50 and n_fused == sum(c.size // c.step <= 64 for c in sc.family("G")) == 34


# ---- streamed calls ----
def pieces_of(c, v, cuts):
    """the reads cut at `cuts`; every second piece shuffled and announced as such"""
    w = sc.weights_for(c.name, len(c.reads), v)
    edges = [0] + sorted(k for k in set(cuts) if 0 < k < len(c.reads)) + [len(c.reads)]
    out = []
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        p = np.random.default_rng(a).permutation(b - a) if i % 2 else np.arange(b - a)
        out.append((np.ascontiguousarray(c.reads[a:b][p]), None if w is None else np.ascontiguousarray(w[a:b][p]), gtx.READS_UNSORTED if i % 2 else 0))
    return out


def test_streamed_calls(engine, beng):
    ran = 0
    for c in sc.family("A") + sc.family("D"):
        cls = c.reads[:, 0]
        change = [int(k) + 1 for k in np.flatnonzero(np.diff(cls) != 0)[:1]]
        for e in (engine, beng):
            for v in DEVICE_VARIANTS:
                for cuts in ((255,), (256,), (257,), tuple(change), (255, 511, 768)):
                    if not cuts:
                        continue
                    for rule, fl in RULES:
                        got = e.scan_stream(pieces_of(c, v, cuts), c.class_len, c.step, c.size, c.prep, weighted=v != "none", flags=fl)[0]
                        np.testing.assert_array_equal(got, expect(c, rule)[v], err_msg="%s/%s streamed, cuts %s, rule %d" % (c.name, v, cuts, rule))
        ran += 1
    assert ran == 41 + 48


# ---- the knobs a process reads once (GTX_SCAN_BUCKETS, GTX_SCAN_FUSED): one fresh child process per knob set ----
def pack_cases(cases):
    """the cases side by side in a few arrays, reads shuffled: (arrays of the .npz, weights as one row per variant of DEVICE_VARIANTS that has weights)"""
    sh = [sc.shuffled(c) for c in cases]
    qoff = np.cumsum([0] + [len(c.reads) for c in cases])
    coff = np.cumsum([0] + [len(c.class_len) for c in cases])
    woff = np.cumsum([0] + [windows(c) for c in cases])
    w = np.stack([np.concatenate([sc.weights_for(c.name, len(c.reads), v)[p] for c, (_, p) in zip(cases, sh)]) for v in DEVICE_VARIANTS if v != "none"])
    return dict(reads=np.concatenate([r for r, _ in sh]), weights=w, reads_off=qoff, class_len=np.concatenate([np.asarray(c.class_len, dtype=np.int32) for c in cases]),
                class_off=coff, win_off=woff, step=np.array([c.step for c in cases]), size=np.array([c.size for c in cases]),
                centre=np.array([c.prep == "c" for c in cases]))


CHILD_SETS = {"buckets-1": ({"GTX_SCAN_BUCKETS": "1"}, "HCG"), "fused-0": ({"GTX_SCAN_FUSED": "0"}, "CG")}


@pytest.mark.parametrize("knobs", sorted(CHILD_SETS))
def test_partition_path_in_a_child_process(knobs, tmp_path):
    env, fams = CHILD_SETS[knobs]
    cases = [c for fam in fams for c in sc.family(fam)]
    assert len(cases) == {"HCG": 45 + 70 + 50, "CG": 70 + 50}[fams]
    packed = pack_cases(cases)
    src, dst = str(tmp_path / "cases.npz"), str(tmp_path / "windows.npy")
    np.savez(src, **packed)
    env = dict(os.environ, GTX_BUCKET_MIN_READS=str(BENG_MIN_READS), **env)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_seams_child.py"), src, dst],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(dst)
    woff = packed["win_off"]
    for i, c in enumerate(cases):
        for k, v in enumerate(DEVICE_VARIANTS):
            np.testing.assert_array_equal(got[k, woff[i]:woff[i + 1]], expect(c, False)[v], err_msg="%s/%s in the child with %s" % (c.name, v, knobs))
