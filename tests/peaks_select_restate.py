"""Restatement of the peak candidate selection (the head of the per-window loop of `genomic_scans peaks`, gtx_peak_select of
include/gtx.h) in numpy -- the reference's gtools/genomic_scans.cpp:304-311, with the window sums read as signed 64-bit values:

    v0 = U ? U[w] : win_size                                   (:304, the mappability track's window, or the window size)
    v1 = min(S[w], v0);  v2 = min(C[w], v0)                    (:305-306)
    norm:  p_ratio < 1.0 ?  v2 = (long)floor((float)v2 * p_ratio)
                         :  v1 = (long)floor((float)v1 / p_ratio)      (:308)
    kept when v1 >= min_reads                                  (:311)

The conversion to float is np.float32 (a count rounds to 24 bits before it is scaled); the product and the quotient are float64, as
the C expression promotes them.  The kept windows come out in window order with the row v1, v2, v0 after clamp and norm."""
import numpy as np


def rows_of(signal, control, uniq, win_size, norm, p_ratio):
    """(n, 3) int64 of v1, v2, v0 for every window"""
    s = np.asarray(signal, dtype=np.uint64).view(np.int64)
    c = np.asarray(control, dtype=np.uint64).view(np.int64)
    assert len(s) == len(c)
    v0 = np.full(len(s), int(win_size), dtype=np.int64) if uniq is None else np.asarray(uniq, dtype=np.uint64).view(np.int64)
    assert len(v0) == len(s)
    v1, v2 = np.minimum(s, v0), np.minimum(c, v0)
    if norm:
        ratio = np.float64(p_ratio)
        if ratio < 1.0:
            v2 = np.floor(v2.astype(np.float32).astype(np.float64) * ratio).astype(np.int64)
        else:
            v1 = np.floor(v1.astype(np.float32).astype(np.float64) / ratio).astype(np.int64)
    return np.stack([v1, v2, v0], axis=1) if len(s) else np.zeros((0, 3), dtype=np.int64)


def select(signal, control, uniq, win_size, min_reads, norm=False, p_ratio=1.0):
    """(ordinals int64, rows int64 [kept, 3]) of the kept windows"""
    rows = rows_of(signal, control, uniq, win_size, norm, p_ratio)
    at = np.flatnonzero(rows[:, 0] >= int(min_reads)).astype(np.int64)
    return at, rows[at]
