"""Restatement of the window filter (`genomic_scans counts -r`, gtx_window_filter of include/gtx.h) in numpy, twice.

Window k (0-based) of a class with step D and size W is [D k + 1, D k + W]; class c has n_windows(class_len[c], D, W) windows at
class_offsets[c] of the vector.  A region (class, s, e) takes part when e >= 1 and s <= e, an s <= 0 counting as 1.  A window is kept
when its value is >= min_value and a region of its class has s <= D k + W and e >= D k + 1; the kept windows come out in vector order.
An ordinal that belongs to no class is never kept.

keep_brute tests every (window, region) pair; keep_runmax sorts a class' regions by start and keeps the running maximum of their
stops: a window [a, b] overlaps a region exactly when j = the number of starts <= b is positive and runmax[j - 1] >= a."""
import numpy as np


def n_windows(length, step, size):
    n, comb = max(int(length), 0) // step, size // step
    return 0 if n < comb else n - comb + 1


def layout(class_len, step, size):
    """(offsets, total) of the classes' windows packed one behind the other"""
    off, tot = [], 0
    for ln in class_len:
        off.append(tot)
        tot += n_windows(ln, step, size)
    return np.asarray(off, dtype=np.int64), tot


def taking_part(refs):
    """the regions that take part, their starts clamped to 1; (n, 3) int64"""
    r = np.asarray(refs, dtype=np.int64).reshape(-1, 3)
    r = r[(r[:, 2] >= 1) & (r[:, 1] <= r[:, 2])].copy()
    r[:, 1] = np.maximum(r[:, 1], 1)
    return r


def _mask_brute(nw, step, size, s, e):
    if nw == 0 or len(s) == 0:
        return np.zeros(nw, dtype=bool)
    a = step * np.arange(nw, dtype=np.int64) + 1
    b = a + size - 1
    return ((s[None, :] <= b[:, None]) & (e[None, :] >= a[:, None])).any(axis=1)


def _mask_runmax(nw, step, size, s, e):
    if nw == 0 or len(s) == 0:
        return np.zeros(nw, dtype=bool)
    order = np.argsort(s, kind="stable")
    s, runmax = s[order], np.maximum.accumulate(e[order])
    a = step * np.arange(nw, dtype=np.int64) + 1
    j = np.searchsorted(s, a + size - 1, side="right")
    return (j > 0) & (runmax[np.maximum(j, 1) - 1] >= a)


def _keep(mask_of, values, class_len, class_off, step, size, refs, min_value):
    values = np.asarray(values, dtype=np.uint64)
    r = taking_part(refs)
    keep = np.zeros(len(values), dtype=bool)
    for c, (ln, off) in enumerate(zip(class_len, class_off)):
        nw = n_windows(ln, step, size)
        mine = r[r[:, 0] == c]
        keep[off:off + nw] |= mask_of(nw, step, size, mine[:, 1], mine[:, 2])
    keep &= values >= np.uint64(min_value)
    at = np.flatnonzero(keep).astype(np.int64)
    return at, values[at]


def keep_brute(values, class_len, class_off, step, size, refs, min_value):
    """(ordinals int64, values uint64) of the kept windows: every pair tested"""
    return _keep(_mask_brute, values, class_len, class_off, step, size, refs, min_value)


def keep_runmax(values, class_len, class_off, step, size, refs, min_value):
    """the same from sorted starts and the running maximum of the stops"""
    return _keep(_mask_runmax, values, class_len, class_off, step, size, refs, min_value)


def random_case(rng, max_windows, max_refs, n_classes=None):
    """a seeded shape: (class_len, step, size, refs) with at most max_windows windows in all; regions of every kind the rule names
    (s <= 0, e <= 0, s > e, duplicates, regions reaching beyond the class), in no order"""
    n_classes = n_classes or int(rng.integers(1, 7))
    step = int(rng.choice([1, 3, 25, 100]))
    size = step * int(rng.choice([1, 2, 20]))
    per = max(max_windows // n_classes, 1)
    class_len = [int(rng.integers(0, per * step + size)) if rng.random() > 0.15 else int(rng.integers(0, size)) for _ in range(n_classes)]
    class_len = [min(ln, (per - 1) * step + size) for ln in class_len]
    n = int(rng.integers(0, max_refs + 1))
    span = max(class_len) + 3 * size + 10
    cls = rng.integers(0, n_classes, size=n)
    s = rng.integers(-size - 5, span, size=n)
    e = s + np.where(rng.random(n) < 0.8, rng.integers(0, 3 * step + 2, size=n), rng.integers(0, span // 3 + 2, size=n)) - (rng.random(n) < 0.1) * 4
    refs = np.stack([cls, s, e], axis=1).astype(np.int64)
    if n > 4:
        refs[rng.integers(0, n, size=n // 8)] = refs[rng.integers(0, n, size=n // 8)]      # duplicates
    return class_len, step, size, refs
