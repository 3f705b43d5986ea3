"""The ticket handshake the text families share (include/gtx.h; csrc/gtx_api_textblock.h): a slot holds one block, of one family.
A family that stages a block into a slot whose unfetched block is another family's ends that block -- its _result finds "no such
block" -- and a family's own unfetched block before last is still refused.  Blocks of one line, through the library directly."""
import ctypes

import pytest

import gtx

pytestmark = pytest.mark.gpu

LINE = b"chr1\t5\t9\n"
SHIFTED = b"chr1\t6\t11\n"                                            # shift 1 2
WINDOWS = b"chr1\t5\t7\nchr1\t7\t9\n"                                 # win -s 2 -d 2
E_STATE = -3                                                          # GTX_E_STATE (include/gtx.h)


def rewrite_send(e, op):
    t = ctypes.c_int(-1)
    rc = e.lib.gtx_rewrite_text(e.ctx, LINE, len(LINE), 1, ctypes.byref(op), ctypes.byref(t))
    return rc, t.value


def rewrite_fetch(e, ticket):
    redo, nb, ns = ctypes.c_int(-1), ctypes.c_size_t(0), ctypes.c_int64(0)
    cap = int(e.lib.gtx_rewrite_max_bytes(len(LINE), 1))
    out = ctypes.create_string_buffer(cap)
    rc = e.lib.gtx_rewrite_result(e.ctx, ticket, ctypes.byref(redo), out, cap, ctypes.byref(nb), ctypes.byref(ns))
    return rc, redo.value, out.raw[:nb.value], ns.value


def windows_send(e, op):
    t = ctypes.c_int(-1)
    rc = e.lib.gtx_windows_text(e.ctx, LINE, len(LINE), 1, ctypes.byref(op), ctypes.byref(t))
    return rc, t.value


def windows_fetch(e, ticket):
    parts = []

    def take(user, p, n):
        parts.append(ctypes.string_at(p, n))
        return 0
    redo, nw, nb = ctypes.c_int(-1), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = e.lib.gtx_windows_result(e.ctx, ticket, ctypes.byref(redo), gtx.LINES_SINK(take), None, ctypes.byref(nw), ctypes.byref(nb))
    return rc, redo.value, b"".join(parts), nw.value


def test_another_familys_block_ends_the_stale_one(engine):
    shift, win = gtx.RewriteOp.make("shift", 1, 2), gtx.WindowsOp.make(2, 2)
    rc, stale = rewrite_send(engine, shift)                           # never fetched
    assert rc == 0 and stale in (0, 1)
    rc, w1 = windows_send(engine, win)
    assert rc == 0 and w1 == stale ^ 1
    rc, w2 = windows_send(engine, win)                                # the stale block's slot: not a rewrite block's refusal
    assert rc == 0 and w2 == stale
    rc = rewrite_fetch(engine, stale)[0]
    assert rc == E_STATE
    assert "gtx_rewrite_result: no such block" in engine.lib.gtx_last_error(engine.ctx).decode()
    assert windows_fetch(engine, w1) == (0, 0, WINDOWS, 2)
    assert windows_fetch(engine, w2) == (0, 0, WINDOWS, 2)
    assert windows_fetch(engine, w2)[0] == E_STATE                    # fetched once


def test_a_familys_own_unfetched_block_is_still_refused(engine):
    shift = gtx.RewriteOp.make("shift", 1, 2)
    rc, t1 = rewrite_send(engine, shift)
    assert rc == 0
    rc, t2 = rewrite_send(engine, shift)
    assert rc == 0 and t2 == t1 ^ 1
    rc, _ = rewrite_send(engine, shift)
    assert rc == E_STATE
    assert "gtx_rewrite_text: the result of the block before last has not been fetched (gtx_rewrite_result)" in engine.lib.gtx_last_error(engine.ctx).decode()
    assert rewrite_fetch(engine, t1) == (0, 0, SHIFTED, 1)
    assert rewrite_fetch(engine, t2) == (0, 0, SHIFTED, 1)
