"""The coverage walk (coverage_walk_body, csrc/gtx_kernels.hip) and the coverage partition kernel (bucket_cover_kernel, csrc/gtx_bucket.hip)
at every step, window, span and bucket seam: the cases of tests/cover_cases.py -- each family aims at one kind of edge and says so in
assertions of its own -- against the brute-force definition cover_cases.brute(), bit for bit, unweighted and with three kinds of weights.
tests/test_cover_cases_cpu.py holds the references against each other and against the oracle, and the kernel constants the cases aim at."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import gtx
import cover_cases as cc

pytestmark = pytest.mark.gpu

WEIGHTED = tuple(v for v in cc.VARIANTS if v != "none")


def make_engine(**env):
    os.environ.update(env)
    try:
        return gtx.Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def eng12():
    e = make_engine(GTX_CHUNKS_PER_WAVE="12")
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng16():
    e = make_engine(GTX_CHUNKS_PER_WAVE="16")
    yield e
    e.close()


@pytest.fixture(scope="module")
def beng():
    e = make_engine(GTX_BUCKET_MIN_READS="1")
    yield e
    e.close()


def device_coverage(e, c):
    import torch
    dev = torch.device("cuda", 0)
    d_reads = torch.from_numpy(np.array(c.reads, dtype=np.int32)).to(dev)
    d_w = None if c.weights is None else torch.from_numpy(np.array(c.weights, dtype=np.int32)).to(dev)
    d_cov = torch.full((max(len(c.refs), 1),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    e.coverage_device(d_reads.data_ptr(), len(c.reads), d_cov.data_ptr(), None if d_w is None else d_w.data_ptr(), c.flags)
    e.sync()
    return d_cov.cpu().numpy().view(np.uint64)[:len(c.refs)]


def check_info(info, c):
    want = cc.expected_info(c)
    assert info["n_no_class"] == want["n_no_class"], c.name
    assert info["n_degenerate"] == want["n_degenerate"], c.name
    if want["first_degenerate"] is not None:
        assert info["first_degenerate"] == want["first_degenerate"], c.name


def check_family(fam, engines, select=None, device=None, info=False, variants=cc.VARIANTS):
    """every case of the family (or those `select` takes) on every context: the regions set once, then each weight variant through the
    host entry (and through coverage_device on the context `device`)"""
    want = cc.wanted(fam)
    ran = 0
    for base in cc.family(fam):
        if select and not select(base):
            continue
        ran += 1
        for tag, e in engines:
            e.set_refs(base.refs, base.n_classes)
            for v in variants:
                c = cc.with_weights(base, v)
                got, inf = e.coverage(c.reads, c.weights, c.flags)
                np.testing.assert_array_equal(got, want[base.name][v], err_msg="%s on %s" % (c.name, tag))
                if info:
                    check_info(inf, c)
                if tag == device:
                    np.testing.assert_array_equal(device_coverage(e, c), want[base.name][v], err_msg="%s on %s, device buffers" % (c.name, tag))
    assert ran
    return ran


def test_a_sizes_and_spans(engine, eng12, eng16):
    check_family("A", [("default", engine), ("cpw12", eng12), ("cpw16", eng16)], device="cpw12")
    check_family("A", [("default", engine)], device="default", variants=("none", "signed"))


@pytest.mark.parametrize("pos", cc.B_POS)
@pytest.mark.parametrize("kind", cc.B_KINDS)
def test_b_boundaries_crossed_by_one_step(engine, eng16, kind, pos):
    tail = "-%s-pos%d" % (kind, pos)
    n = check_family("B", [("default", engine), ("cpw16", eng16)], select=lambda c: c.name.endswith(tail), device="cpw16")
    assert n == len(cc.B_P) * len(cc.B_C)


def test_c_crossings_without_a_step(engine):
    check_family("C", [("default", engine)])


def test_d_equal_keys_and_thresholds(engine, eng16):
    check_family("D", [("default", engine), ("cpw16", eng16)])


def test_e_spread_and_coordinate_limits(engine, eng16):
    check_family("E", [("default", engine), ("cpw16", eng16)], device="default")


@pytest.mark.parametrize("kind", cc.F_KINDS)
def test_f_what_refuses_a_step(engine, kind):
    n = check_family("F", [("default", engine)], select=lambda c: c.name.startswith("F-%s-pos" % kind), info=True)
    assert n == len(cc.F_POS)


def test_g_classes_and_histogram_tiles(engine, eng16):
    check_family("G", [("default", engine), ("cpw16", eng16)])


# ---- H: streamed calls ----
H_EDGES = (1, 63, 64, 255, 256, 257, 511)


def streamed(e, c, cuts):
    """gtx_coverage_begin / _add per batch / _end; cuts = the read indices at which a new batch begins"""
    lib, reads = e.lib, np.ascontiguousarray(c.reads, dtype=np.int32)
    w = None if c.weights is None else np.ascontiguousarray(c.weights, dtype=np.int32)
    e._chk(lib.gtx_coverage_begin(e.ctx))
    edges = [0] + [k for k in cuts if 0 < k < len(reads)] + [len(reads)]
    for a, b in zip(edges[:-1], edges[1:]):
        r = np.ascontiguousarray(reads[a:b])
        ww = None if w is None else np.ascontiguousarray(w[a:b])
        e._chk(lib.gtx_coverage_add(e.ctx, gtx._ptr(r), gtx._ptr(ww), b - a, int(c.flags)))
    cov = np.zeros(max(len(c.refs), 1), dtype=np.uint64)
    info = gtx.CountInfo()
    e._chk(lib.gtx_coverage_end(e.ctx, gtx._ptr(cov), ctypes.byref(info)))
    return cov[:len(c.refs)], info.as_dict()


@pytest.mark.parametrize("variant", cc.VARIANTS)
def test_h_streamed_calls_equal_the_one_shot_call(engine, variant):
    want = cc.wanted("A")
    for base in cc.family("A"):
        c = cc.with_weights(base, variant)
        engine.set_refs(c.refs, c.n_classes)
        one, _ = engine.coverage(c.reads, c.weights, c.flags)
        np.testing.assert_array_equal(one, want[base.name][variant], err_msg=c.name)
        for cuts in [(b,) for b in H_EDGES] + [tuple(np.cumsum(H_EDGES).tolist())]:
            for again in range(2):                                 # back to back on one context: the state was zeroed
                got, _ = streamed(engine, c, cuts)
                np.testing.assert_array_equal(got, one, err_msg="%s streamed with cuts %s, call %d" % (c.name, cuts, again))


def test_h_first_degenerate_is_a_global_index_in_the_second_batch(engine):
    for base in cc.family("F"):
        if "inverted" not in base.name:
            continue
        engine.set_refs(base.refs, base.n_classes)
        for cut in (cc.STEP, cc.STEP + 100):
            got, info = streamed(engine, base, (cut,))
            np.testing.assert_array_equal(got, cc.wanted("F")[base.name]["none"], err_msg=base.name)
            check_info(info, base)


# ---- I: the partition kernel ----
def test_i_partition_kernel(beng):
    check_family("I", [("bucket", beng)])
    for base in cc.family("I")[:3]:                                 # (coverRule: inverted reads are reported, zero-length ones dropped silently)
        beng.set_refs(base.refs, base.n_classes)
        _, info = beng.coverage(base.reads, None, base.flags)
        check_info(info, base)


# ---- the general weighted code (GTX_WEIGHTED_FAST=0, read once per process): one child process ----
def pack_cases(cases):
    """the cases side by side in a few arrays: (arrays of the .npz, weights as one row per weighted variant)"""
    roff = np.cumsum([0] + [len(c.refs) for c in cases])
    qoff = np.cumsum([0] + [len(c.reads) for c in cases])
    w = np.stack([np.concatenate([cc.weights_for(c.name, len(c.reads), v) for c in cases]) for v in WEIGHTED])
    return dict(refs=np.concatenate([c.refs for c in cases]), reads=np.concatenate([c.reads for c in cases]), weights=w, refs_off=roff, reads_off=qoff,
                n_classes=np.array([c.n_classes for c in cases]), flags=np.array([c.flags for c in cases]))


def test_weighted_general_code_in_a_child_process(engine, tmp_path):
    cases = [c for fam in "ABDF" for c in cc.family(fam)]
    packed = pack_cases(cases)
    src, dst = str(tmp_path / "cases.npz"), str(tmp_path / "general.npy")
    np.savez(src, **packed)
    env = dict(os.environ, GTX_WEIGHTED_FAST="0")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "cover_general_child.py"), src, dst],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    general = np.load(dst)
    roff = packed["refs_off"]
    for i, c in enumerate(cases):
        want = cc.wanted(c.name[0])[c.name]
        for k, v in enumerate(WEIGHTED):
            got = general[k, roff[i]:roff[i + 1]]
            np.testing.assert_array_equal(got, want[v], err_msg="%s/%s through the general code" % (c.name, v))
            if k == 0:
                engine.set_refs(c.refs, c.n_classes)
            fast, _ = engine.coverage(c.reads, cc.weights_for(c.name, len(c.reads), v), c.flags)
            np.testing.assert_array_equal(got, fast, err_msg="%s/%s: the general code against the fast path" % (c.name, v))
