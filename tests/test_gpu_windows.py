"""gtx_windows_text / gtx_windows_result (include/gtx.h; kernels csrc/gtx_windows.hip) through Engine.windows_text against the
restatement (tests/windows_restate.py), byte for byte: blocks whose line counts sit on the lane, wave and line-tile seams, lines
whose windows sit on the output-tile seams, starts and stops that cross every power of ten on and beside a tile boundary, the
clipped tail of --small, lines without a window wherever a tile can have them, every column count, runs that start at every residue
mod 16, ranges of one tile, a sink that refuses, two blocks in flight, a skewed block, and the blocks that must come back.  Line tile
T, output tile W and the longest fixed part F come from gtx_windows_limits."""
import numpy as np
import pytest

import gtx
import windows_restate as wr

pytestmark = pytest.mark.gpu

DEFAULT_CHUNK = 64 << 20                                               # gtx_set_lines_chunk's default (include/gtx.h)
ZERO = "chr1\t5\t5"                                                    # START = 6 > STOP: no window


@pytest.fixture(scope="module")
def limits():
    T, W, F = gtx.windows_limits()
    assert T >= 64 and T % 64 == 0 and W >= 64 and F >= 32
    return T, W, F


def op_of(step, size, small=False):
    return {"step": step, "size": size, "small": small}


def check(engine, op, blocks, chunk=None):
    """every block expanded as the restatement expands it; the totals are the text's own"""
    try:
        got = engine.windows_text([b.encode() for b in blocks], gtx.WindowsOp.make(op["size"], op["step"], op["small"]), chunk=chunk)
    finally:
        if chunk is not None:
            engine.set_lines_chunk(DEFAULT_CHUNK)
    assert len(got) == len(blocks)
    for b, (redo, text, n, calls) in zip(blocks, got):
        assert all(wr.is_plain(l) for l in b.split("\n")[:-1])
        want = wr.run(op, b)[0]
        assert redo == 0
        assert text.decode() == want
        assert n == want.count("\n")
        assert (calls == 0) == (want == "")
    return got


def block(lines):
    return "".join(l + "\n" for l in lines)


def line_with(n, step, size, v2=1000, cols=4, name="chr1"):
    """a plain line with exactly n full-size windows (n >= 1)"""
    return "\t".join([name, str(v2), str(v2 + size + (n - 1) * step), "w%d" % n, "7", "-"][:cols])


def short_lines(seed, n):
    """n plain lines of 3 to 6 columns with 0 to 3 windows of -s 25 -d 25 each"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        s = int(rng.integers(0, 3_000_000))
        cols = ["chr%d" % rng.integers(1, 23), str(s), str(s + int(rng.integers(0, 100))), "r%d" % k, str(int(rng.integers(-5, 1000))), "+-"[int(rng.integers(0, 2))]]
        out.append("\t".join(cols[:int(rng.integers(3, 7))]))
    return out


def test_blocks_on_the_line_seams(engine, limits):
    T, W, F = limits
    sizes = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    blocks = [block(short_lines(20 + k, n)) for k, n in enumerate(sizes)]
    want = [wr.run(op_of(25, 25), b)[0].count("\n") for b in blocks]
    assert want[-1] > W                                                # more than one output tile
    check(engine, op_of(25, 25), blocks)
    check(engine, op_of(25, 25, True), blocks)


def test_one_line_on_the_output_tile_seams(engine, limits):
    T, W, F = limits
    blocks = []
    for n in (W - 1, W, W + 1, 3 * W + 1):
        blocks.append(block([line_with(n, 7, 10)]))
        blocks.append(block([ZERO] * 3 + [line_with(n, 7, 10)] + [ZERO] * (T + 2)))
    check(engine, op_of(7, 10), blocks)


@pytest.mark.parametrize("step", [1, 7, 10 ** 4])
def test_powers_of_ten_on_and_beside_a_tile_boundary(engine, limits, step):
    """the start column reaches 10^j at window 2 W + delta of its block, the stop column at window W + delta"""
    T, W, F = limits
    size = step * W
    blocks = []
    for j in range(1, 10):
        for delta in (-1, 0, 1):
            v2 = 10 ** j - step * (2 * W + delta)
            if v2 < 0:
                v2 = 10 ** j % step                                    # the crossing comes as early as the step lets it
            b = block([line_with(3 * W + 5, step, size, v2=v2, cols=3 + (j + delta) % 4)])
            rows = wr.run(op_of(step, size), b)[0].split("\n")[:-1]
            starts = [len(r.split("\t")[1]) for r in rows]
            k = next(i for i in range(1, len(rows)) if starts[i] > starts[i - 1]) if starts[-1] > starts[0] else None
            if 10 ** j >= step * (2 * W + 1):
                assert k == 2 * W + delta
            blocks.append(b)
    check(engine, op_of(step, size), blocks)


def test_the_clipped_tail_of_small(engine, limits):
    T, W, F = limits
    blocks = [block([ZERO, "chr2\t990\t%d\tx\t1\t+" % (990 + length), "chr3\t0\t7"]) for length in (1500, W + 998, W + 999, W + 1000, 5, 999, 1000, 1001)]
    first = wr.run(op_of(1, 1000, True), blocks[0])[0].split("\n")[:-1]
    assert len(first) == 1507 and sum(r.startswith("chr2") and r.split("\t")[2] == "2490" for r in first) == 1000   # 999 of them clipped
    check(engine, op_of(1, 1000, True), blocks)
    check(engine, op_of(1, 1000, False), blocks)
    check(engine, op_of(3, 1000, True), blocks)


def test_lines_without_a_window(engine, limits):
    T, W, F = limits
    one = line_with(1, 5, 5)
    got = check(engine, op_of(5, 5), [block([ZERO] * T), block([ZERO]), block([ZERO] * (3 * T + 7))])
    assert all(g == (0, b"", 0, 0) for g in got)                        # no window: no sink call
    check(engine, op_of(5, 5), [block([ZERO] * T + [one] * T), block([one] * T + [ZERO] * T), block([ZERO] + [one] * (T - 2) + [ZERO]),
                                block([ZERO] * (5 * T) + [one] + [ZERO] * (5 * T) + [line_with(W + 3, 5, 5)] + [ZERO] * T),
                                block(([ZERO] * 9 + [one]) * 300)])    # one tile of windows across 3000 lines


def test_every_column_count(engine):
    b = block(["chr1\t0\t10", "chr1\t0\t10\tlab", "chr1\t0\t10\tlab\t77", "chr1\t0\t10\tlab\t-77\t-", "chrUn_gl000220\t100\t161\tlabel_with_length\t0\t+"])
    got = check(engine, op_of(5, 5), [b])
    assert got[0][1].decode().startswith("chr1\t0\t5\nchr1\t5\t10\nchr1\t0\t5\tlab\nchr1\t5\t10\tlab\nchr1\t0\t5\tlab\nchr1\t5\t10\tlab\nchr1\t0\t5\tlab\t-77\t-\n")
    check(engine, op_of(3, 4, True), [b])


def test_runs_start_at_every_residue_mod_16(engine, limits):
    T, W, F = limits
    blocks, seen = [], set()
    for r in range(16):
        b = block(["c" * (r + 1) + "\t10\t20\tz", line_with(2 * W + 9, 10, 10, v2=100_000)])
        rows = wr.run(op_of(10, 10), b)[0].split("\n")[:-1]
        seen.add(sum(len(x) + 1 for x in rows[:W]) % 16)
        blocks.append(b)
    assert seen == set(range(16))                                     # where the second tile's run begins
    check(engine, op_of(10, 10), blocks)


def test_ranges_of_one_tile(engine, limits):
    """the lines chunk at one tile's bound: every range is one tile, and a line's windows straddle ranges"""
    T, W, F = limits
    b = block(short_lines(7, 300) + [line_with(3 * W + 1, 7, 10)] + short_lines(8, 2 * T))
    total = wr.run(op_of(7, 10, True), b)[0].count("\n")
    got = check(engine, op_of(7, 10, True), [b, b], chunk=1)
    assert total > 4 * W and all(g[3] == (total + W - 1) // W for g in got)
    got = check(engine, op_of(7, 10, True), [b], chunk=2 * W * (F + 20))
    assert got[0][3] == ((total + W - 1) // W + 1) // 2


def test_a_sink_that_refuses_its_third_call(engine, limits):
    T, W, F = limits
    b = block([line_with(5 * W, 7, 10)] + short_lines(9, 50))
    op = gtx.WindowsOp.make(10, 7)
    try:
        with pytest.raises(gtx.GtxError, match=r"gtx error %d: .*sink refused" % gtx.E_SINK):
            engine.windows_text([b.encode(), b.encode(), b.encode()], op, chunk=1, refuse_at=3)
        check(engine, op_of(7, 10), [b, b], chunk=1)                  # the context is usable afterwards
    finally:
        engine.set_lines_chunk(DEFAULT_CHUNK)
    check(engine, op_of(7, 10), [b])


def test_two_blocks_in_flight(engine, limits):
    T, W, F = limits
    blocks = [block(short_lines(30 + k, n) + [line_with(m, 25, 25)]) for k, (n, m) in enumerate([(5, 1), (2 * T, 2 * W), (1, 3), (T + 1, W + 1), (700, 9)])]
    got = check(engine, op_of(25, 25), blocks)
    assert len({g[1] for g in got}) == len(blocks)


def test_a_skewed_block(engine):
    """one line with 10^6 windows among 10^4 lines with one window each"""
    lines = [line_with(1, 25, 25, v2=100 * k, cols=3 + k % 4, name="chr%d" % (1 + k % 22)) for k in range(10_000)]
    lines.insert(5_000, line_with(10 ** 6, 25, 25, v2=999_000, cols=6, name="chr9"))
    got = check(engine, op_of(25, 25), [block(lines)])
    assert got[0][2] == 10 ** 6 + 10 ** 4


def test_blocks_that_come_back(engine, limits):
    T, W, F = limits
    good = short_lines(3, 40)
    long_fixed = "chrom12345\t0\t100\t" + "L" * (F - 14 + 1)             # a fixed part of F + 1 bytes
    assert wr.fixed_part(long_fixed) == F + 1
    for odd in ("chr1 0 100 x 1 +", "chr1\t0\t100\tx\t1\t+\t5", "chr1\t0\t100\tx\t1\t.", long_fixed):
        got = engine.windows_text([block(good[:20] + [odd] + good[20:]).encode(), block(good).encode()], gtx.WindowsOp.make(25, 25))
        assert got[0][0] != 0 and got[0][1:] == (b"", 0, 0)            # no sink call, zero totals
        assert got[1][0] == 0 and got[1][1].decode() == wr.run(op_of(25, 25), block(good))[0]


def test_a_fixed_part_of_exactly_the_limit_stays(engine, limits):
    T, W, F = limits
    exact = "chrom12345\t0\t100\t" + "L" * (F - 14)
    assert wr.fixed_part(exact) == F
    six = "chrom12345\t0\t100000\t" + "L" * (F - 18) + "\t5\t-"
    assert wr.fixed_part(six) == F
    check(engine, op_of(25, 25), [block([exact]), block([exact] * (T + 1) + [six])])
    big = "chrom12345\t1000000000\t2000000000\t" + "L" * (F - 18) + "\t5\t-"
    got = check(engine, op_of(10 ** 6 - 1, 999_000, True), [block([big] * 3)])   # F + 20 bytes a window: whole tiles fill their bound
    assert got[0][2] > 2 * W and all(len(r) + 1 == F + 20 for r in got[0][1].decode().split("\n")[:-1])


def test_sizes_and_steps_the_device_does_not_take(engine):
    for size, step in ((0, 1), (1, 0), (-3, 1), (2 ** 31 + 1, 1), (1, 2 ** 31 + 1)):
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            engine.windows_text([b"chr1\t0\t10\n"], gtx.WindowsOp.make(size, step))
    check(engine, op_of(2 ** 31, 2 ** 31, True), [block(["chr1\t0\t2147483645", "chr1\t5\t9\tx"])])
    check(engine, op_of(2 ** 31, 1, True), [block(["chr1\t2147483000\t2147483645\ty\t1\t+"])])
