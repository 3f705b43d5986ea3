"""CPU suite: the two numpy restatements of the window filter (tests/window_filter_restate.py) against each other on seeded shapes, and
against the oracle CLI's `counts -r` on a small BED -- the window sums taken from the oracle's plain `counts -min 0` run, so that only
the filter is under test.  The yardstick the device filter (tests/test_gpu_window_filter.py) is held to."""
import numpy as np
import pytest

import window_filter_restate as wf
from oracle import orc

NAMES = ["chrA", "chrB", "chrC"]                                                 # in strcmp order
LENGTHS = [60000, 9000, 90]


def test_the_two_restatements_agree_on_seeded_shapes():
    rng = np.random.default_rng(41)
    kept = 0
    for _ in range(200):
        class_len, step, size, refs = wf.random_case(rng, 600, 120)
        off, tot = wf.layout(class_len, step, size)
        values = rng.integers(0, 6, size=tot).astype(np.uint64)
        for min_value in (0, 1, 3, 7):
            a = wf.keep_brute(values, class_len, off, step, size, refs, min_value)
            b = wf.keep_runmax(values, class_len, off, step, size, refs, min_value)
            np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
            kept += len(a[0])
    assert kept > 10000


def test_edges_by_hand():
    # one class of length 100, step 10, size 20: windows k = 0 .. 8 are [10 k + 1, 10 k + 20]
    values = np.full(9, 5, dtype=np.uint64)
    def kept(refs, min_value=0):
        a = wf.keep_brute(values, [100], [0], 10, 20, refs, min_value)[0].tolist()
        assert a == wf.keep_runmax(values, [100], [0], 10, 20, refs, min_value)[0].tolist()
        return a
    assert kept([[0, 40, 40]]) == [2, 3]                            # s = D k + W of window 2: kept; window 1 ends at 30
    assert kept([[0, 41, 41]]) == [3, 4]                            # s = D k + W + 1 of window 2: not kept
    assert kept([[0, 1, 31]]) == [0, 1, 2, 3]                       # e = D k + 1 of window 3: kept
    assert kept([[0, 1, 30]]) == [0, 1, 2]                          # e = D k of window 3: not kept
    assert kept([[0, -7, 1]]) == [0] and kept([[0, 0, 0]]) == [] and kept([[0, -3, -1]]) == [] and kept([[0, 50, 49]]) == []
    assert kept([[0, 5, 95], [0, 6, 7], [0, 8, 9], [0, 10, 11]]) == list(range(9))   # the long region behind the short ones: running maximum
    assert kept([[0, 40, 40]], 6) == [] and kept([[0, 40, 40]], 5) == [2, 3]


@pytest.fixture(scope="module")
def beds(tmp_path_factory):
    d = tmp_path_factory.mktemp("wf")
    rng = np.random.default_rng(42)
    with open(d / "genome.bed", "w") as f:
        for n, ln in zip(NAMES, LENGTHS):
            f.write("%s\t0\t%d\n" % (n, ln))
    lines = []
    for _ in range(8000):
        c = int(rng.integers(0, 3))
        s = int(rng.integers(1, LENGTHS[c] + 200))
        lines.append("%s\t%d\t%d\tr\t0\t%s" % (NAMES[c], s - 1, s + 30, "+-"[int(rng.integers(0, 2))]))
    (d / "reads.bed").write_text("\n".join(lines) + "\n")
    refs = []                                                                  # (chromosome, strand, start, stop), 1-based inclusive
    for _ in range(60):
        c = int(rng.integers(0, 2))
        s = int(rng.integers(1, LENGTHS[c] + 300))
        refs.append((c, int(rng.integers(0, 2)), s, s + int(rng.integers(0, 120))))
    refs += [(0, 0, 1000, 1000), (0, 0, 1000, 1000), (0, 1, 1501, 1501), (0, 0, 2001, 2001), (1, 1, 1, 1), (1, 0, 9000, 9100), (0, 0, 3000, 4200), (0, 0, 3010, 3011),
             (0, 0, 3020, 3021), (2, 0, 10, 20)]
    refs = [refs[k] for k in rng.permutation(len(refs))]
    (d / "refs.bed").write_text("".join("%s\t%d\t%d\tg%d\t0\t%s\n" % (NAMES[c], s - 1, e, k, "+-"[m]) for k, (c, m, s, e) in enumerate(refs)))
    return d, refs


def windows_of(d, args):
    """the oracle's window sums for a geometry, as (values in print order, lines by ordinal)"""
    rc, out, err = orc.cli(["counts"] + args + ["-min", "0", "-g", str(d / "genome.bed"), str(d / "reads.bed")])
    assert rc == 0, err
    lines = out.splitlines(keepends=True)
    return np.array([int(x.split("\t")[0]) for x in lines], dtype=np.uint64), lines


@pytest.mark.parametrize("ignore_strand", [False, True], ids=["stranded", "-i"])
@pytest.mark.parametrize("step,size", [(25, 500), (100, 100), (10, 20)])
@pytest.mark.parametrize("min_value", [0, 1, 12])
def test_restatements_give_the_oracle_clis_filtered_output(beds, ignore_strand, step, size, min_value):
    d, refs = beds
    geom = (["-i"] if ignore_strand else []) + ["-w", str(size), "-d", str(step)]
    values, lines = windows_of(d, geom)
    ns = 1 if ignore_strand else 2
    class_len = [LENGTHS[b // ns] for b in range(len(NAMES) * ns)]                  # a class per printed block: chromosome, then strand
    off, tot = wf.layout(class_len, step, size)
    assert tot == len(values)
    tri = [[c * ns + (0 if ignore_strand else m), s, e] for c, m, s, e in refs]
    rc, out, err = orc.cli(["counts"] + geom + ["-min", str(min_value), "-r", str(d / "refs.bed"), "-g", str(d / "genome.bed"), str(d / "reads.bed")])
    assert rc == 0, err
    for keep in (wf.keep_brute, wf.keep_runmax):
        at, v = keep(values, class_len, off, step, size, tri, min_value)
        assert "".join(lines[k] for k in at) == out
        assert 0 < len(at) < tot
