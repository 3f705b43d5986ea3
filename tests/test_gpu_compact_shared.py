"""The window selection, the window filter and the peak candidate selection taking turns on one context: the three are rules of one
tile compaction (csrc/gtx_compact.h) and share the context's scratch -- tile counts and bases, the ordinals and one row buffer sized
in bytes, reused here at 16, 8 and 24 bytes a row.  The expected answers are the restatements' (the numpy statement of the table
rule that test_gpu_window_select.py checks against -- tests/peakdiff_restate.py states that rule on files, not on vectors --,
tests/window_filter_restate.py, tests/peaks_select_restate.py), and every call is repeated on a context that has run nothing else."""
import numpy as np
import pytest
import torch

import gtx
import peaks_select_restate as ps
import window_filter_restate as wf
from test_gpu_window_select import random_case, rule

pytestmark = pytest.mark.gpu

TILE = gtx.window_select_limits()[0]
SENTINEL = -7


def on_device(v):
    a = np.ascontiguousarray(v, dtype=np.uint64)
    return torch.from_numpy(np.concatenate([a, np.zeros(2, dtype=np.uint64)]).view(np.int64)).cuda()


class Select:
    """2 tested vectors with controls, n = 3 TILE + 7: rows of 4 int32"""
    row_dtype, row_cols = np.int32, 4

    def __init__(self):
        self.n, self.W = 3 * TILE + 7, 20
        self.tested, self.controls, self.tables = random_case(41, self.n, 2, True, self.W)
        self.want = rule(self.tested, self.controls, self.tables, self.W)
        self.dt, self.dc = [on_device(v) for v in self.tested], [on_device(v) for v in self.controls]

    def call(self, eng, capacity=None, device_out=None):
        return eng.window_select([t.data_ptr() for t in self.dt], self.tables, self.W, controls=[t.data_ptr() for t in self.dc], n_windows=self.n,
                                 capacity=capacity, device_out=device_out)


class Filter:
    """one class of TILE - 1 windows: rows of one uint64"""
    row_dtype, row_cols = np.uint64, 1

    def __init__(self):
        self.n, self.step, self.size = TILE - 1, 25, 50
        self.class_len = [(self.n - 1) * self.step + self.size]
        assert wf.n_windows(self.class_len[0], self.step, self.size) == self.n
        rng = np.random.default_rng(42)
        self.values = rng.integers(0, 4, size=self.n).astype(np.uint64)
        s = rng.integers(1, self.class_len[0], size=60)
        self.refs = np.stack([np.zeros(60, dtype=np.int64), s, s + rng.integers(0, 3 * self.step, size=60)], axis=1)
        self.off = np.zeros(1, dtype=np.int64)
        o, v = wf.keep_brute(self.values, self.class_len, self.off, self.step, self.size, self.refs, 1)
        self.want = (o, v.reshape(-1, 1))
        self.d = on_device(self.values)

    def call(self, eng, capacity=None, device_out=None):
        eng.window_refs(self.refs, self.class_len, self.off, self.step, self.size)
        got = eng.window_filter(self.d.data_ptr(), 1, n_windows=self.n, capacity=capacity, device_out=device_out)
        return got if device_out is not None else (got[0], got[1].reshape(-1, 1), got[2])


class Peaks:
    """n = 5 TILE + 1 with the mappability vector: rows of 3 int64"""
    row_dtype, row_cols = np.int64, 3

    def __init__(self):
        self.n = 5 * TILE + 1
        rng = np.random.default_rng(43)
        self.S, self.C, self.U = (rng.integers(0, 30, size=self.n).astype(np.uint64) for _ in range(3))
        self.want = ps.select(self.S, self.C, self.U, 20, 12, True, 0.37)
        self.dS, self.dC, self.dU = on_device(self.S), on_device(self.C), on_device(self.U)

    def call(self, eng, capacity=None, device_out=None):
        args = dict(uniq=self.dU.data_ptr(), norm=True, p_ratio=0.37, n_windows=self.n)
        if device_out is not None:
            return eng.peak_select_device(self.dS.data_ptr(), self.dC.data_ptr(), 20, 12, capacity, device_out[0], device_out[1], **args)
        return eng.peak_select(self.dS.data_ptr(), self.dC.data_ptr(), 20, 12, capacity=capacity, **args)


def same(got, want_o, want_r, n_kept):
    o, r, kept = got
    assert kept == n_kept
    np.testing.assert_array_equal(o, want_o)
    np.testing.assert_array_equal(np.asarray(r).reshape(len(want_o), -1), want_r)


def on_a_fresh_engine(case, capacity):
    e = gtx.Engine(0)
    try:
        got = case.call(e, capacity)
        torch.cuda.synchronize()
        return got
    finally:
        e.close()


def test_three_selectors_take_turns_on_one_context():
    cases = [Select(), Filter(), Peaks()]
    for c in cases:
        assert 2 < len(c.want[0]) < c.n and c.want[1].shape == (len(c.want[0]), c.row_cols)
    eng = gtx.Engine(0)
    try:
        for short in (0, 1):                                                     # the second round: one row less room than is kept
            for c in cases:
                want_o, want_r = c.want
                kept = len(want_o)
                cap = kept - 1 if short else None
                got = c.call(eng, cap)
                torch.cuda.synchronize()
                same(got, want_o[:cap], want_r[:cap], kept)
                same(on_a_fresh_engine(c, cap), got[0], np.asarray(got[1]).reshape(len(got[0]), -1), kept)
                if not short:
                    continue
                # the device entry with the same room: the exact prefix, and nothing behind the capacity
                d_o = torch.full((kept + 64,), SENTINEL, dtype=torch.int64, device="cuda")
                d_r = torch.from_numpy(np.full((kept + 64) * c.row_cols, SENTINEL, dtype=np.int64).astype(c.row_dtype).view(np.uint8)).cuda()
                assert c.call(eng, cap, (d_o.data_ptr(), d_r.data_ptr())) == kept
                torch.cuda.synchronize()
                ho, hr = d_o.cpu().numpy(), d_r.cpu().numpy().view(c.row_dtype)
                np.testing.assert_array_equal(ho[:cap], want_o[:cap])
                np.testing.assert_array_equal(hr[:cap * c.row_cols].reshape(-1, c.row_cols), want_r[:cap])
                assert (ho[cap:] == SENTINEL).all() and (hr[cap * c.row_cols:] == np.int64(SENTINEL).astype(c.row_dtype)).all()
    finally:
        eng.close()
