"""gtx_blocks_text / gtx_blocks_result (include/gtx.h; kernels csrc/gtx_blocks.hip) through the C ABI against the restatement
(tests/blocks_restate.py), byte for byte, for split, connect, select, diff, n and strand: blocks whose line counts sit on the lane
and tile seams, block counts up to max_blocks, 3-to-6- and 12-column lines inside one tile, runs that start at every residue mod 16
of the output, the digit-count seams of every rendered number, labels, names and colours of one byte and as long as the stage lets
them be, a tile whose run just fits and just misses the stage, select's 16 flag combinations, diff lines, tiles and blocks that
print nothing, split lines whose outputs straddle emit tiles, both spellings of the lists, one odd line in one of three blocks, the
sink called in pieces that end at a line's end, the manifest's plain cases and the argument errors.  Tile, stage and max_blocks come
from gtx_blocks_limits.  (The result reaches the caller through a sink, in pieces of the library's own page-locked buffer: there is
no caller's buffer to put a canary behind; what is checked instead is that the sink is given exactly n_bytes bytes, which
Engine.blocks_text raises on, and that they are the restatement's.)"""
import json
import os
import random

import pytest

import blocks_cases as bc
import blocks_restate as br
import gtx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "blocks_manifest.json")))["cases"]
OPS = bc.ops()
ONE_LINE_OPS = [o for o in OPS if o["kind"] != "split"]
TOP = 2 ** 31 - 3                                                     # the largest plain coordinate
OUT_TILE = 256                                                        # split: printed lines per emit block (csrc/gtx_blocks.h)
DEFAULT_CHUNK = 64 << 20                                              # gtx_set_lines_chunk's default (include/gtx.h)

every_op = pytest.mark.parametrize("op", OPS, ids=bc.op_id)
one_line_op = pytest.mark.parametrize("op", ONE_LINE_OPS, ids=bc.op_id)


def device_op(op):
    sel = sum(bit for f, bit in zip(br.SELECT_FLAGS, (gtx.BLOCKS_FIRST, gtx.BLOCKS_LAST, gtx.BLOCKS_5P, gtx.BLOCKS_3P)) if op[f])
    return gtx.BlocksOp.make(op["kind"], sel, op["op"])


def check(engine, op, blocks):
    """every block printed as the restatement prints it"""
    for b in blocks:
        assert all(br.is_plain(l) for l in b.split("\n")[:-1])
    got = engine.blocks_text([b.encode() for b in blocks], device_op(op))
    assert len(got) == len(blocks)
    for b, (redo, text, n, calls) in zip(blocks, got):
        want, err, code = br.run(op, b)
        assert (err, code) == ("", 0)
        assert redo == 0
        assert text.decode() == want
        assert n == want.count("\n")
        assert calls == (1 if want else 0)
    return got


def line12(label="l", name="c", rgb="0", k=0, sizes=(10, 20), starts=(0, 40), start=100, strand=None, thick=None, comma=None):
    """a plain 12-column line: two blocks with a gap between them unless told otherwise"""
    z = start + starts[-1] + sizes[-1]
    return bc.bed12(name, start + 0, label, str(k), strand or "+-"[k & 1], thick or (min(start + 5, z), max(z - 5, start)), rgb, list(sizes), list(starts), comma=bool(k & 1) if comma is None else comma)


@pytest.fixture(scope="module")
def limits():
    tile, stage, max_blocks = gtx.blocks_limits()
    assert tile >= 64 and tile % 64 == 0 and stage >= 16 * tile and max_blocks >= 1024 and max_blocks == br.MAX_BLOCKS
    return tile, stage, max_blocks


@every_op
def test_block_sizes_two_in_flight(engine, limits, op):
    T = limits[0]
    rng = random.Random(41)
    sizes = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    blocks = [bc.text_of([bc.plain(rng) for _ in range(n)]) for n in sizes]     # (eight blocks, two in flight, fetched in order)
    first = blocks[-1].split("\n")[:T]
    assert any(len(l.split("\t")) == 12 for l in first) and any(len(l.split("\t")) < 12 for l in first)   # both kinds of line inside one tile
    check(engine, op, blocks)


@every_op
def test_block_counts_up_to_max_blocks(engine, limits, op):
    T, _, M = limits
    rng = random.Random(43)
    lines = []
    for n in (1, 2, 3, 63, 64, 65, M - 1, M):
        for comma in (False, True):
            lines.append(bc.plain12(rng, n, comma=comma, max_gap=60, max_size=90))
            lines.append(bc.plain_short(rng))
    assert {l.split("\t")[10].endswith(",") for l in lines if len(l.split("\t")) == 12} == {False, True}
    check(engine, op, [bc.text_of(lines)])
    small = bc.text_of([bc.plain(rng) for _ in range(T + 3)])
    over = bc.plain12(rng, M + 1, max_gap=60, max_size=90)
    assert not br.is_plain(over)
    got = engine.blocks_text([small.encode(), bc.text_of(lines + [over]).encode(), small.encode()], device_op(op))
    assert got[1][0] != 0 and got[1][1:] == (b"", 0, 0)
    for k in (0, 2):
        assert got[k][0] == 0 and got[k][1].decode() == br.run(op, small)[0]


@every_op
def test_runs_start_at_every_residue_of_the_output(engine, limits, op):
    T = limits[0]
    split = op["kind"] == "split"
    n_first = OUT_TILE // 2 if split else T                              # the input lines in front of the second run (split: two printed lines each)
    rest = [line12("l%d" % k, "chr2", k=k) for k in range(1, 3 * OUT_TILE)]
    # the first line prints its label once, so the second run starts one byte later with every byte of it
    first = (lambda r: "\t".join(["chr2", "100", "160", "L" * r, "0", "+"])) if split else (lambda r: line12("L" * r, "chr2", k=0, strand="+"))
    blocks = [bc.text_of([first(r)] + rest) for r in range(1, 17)]
    check(engine, op, blocks)
    if split:
        starts = {len("".join(br.run(op, b)[0].splitlines(True)[:OUT_TILE])) % 16 for b in blocks}
    else:
        starts = {len(br.run(op, bc.text_of(b.split("\n")[:n_first]))[0]) % 16 for b in blocks}
    assert starts == set(range(16))


@every_op
def test_digit_count_seams_of_every_rendered_number(engine, limits, op):
    edges = sorted({1, 2} | {10 ** j + d for j in range(1, 10) for d in (-1, 0, 1)})
    lines, k = [], 0
    for v in [0] + edges:
        lines.append("chr1\t%d\t%d" % (v, v + 1))                       # START-1 and STOP of a short line
        lines.append("chr1\t%d\t%d\tb%d\t%d\t-" % (max(v - 3, 0), v + 1, k, k))
        lines.append(line12(k=k, start=v, sizes=(1, 1), starts=(0, 5)))            # START-1 of every block
        k += 1
    for v in edges:
        lines.append(line12(k=k, start=0, sizes=(v, 3), starts=(0, v + 2)))        # a size, the start behind it, the stops
        lines.append(line12(k=k, start=0, sizes=(1, 1), starts=(0, v)))            # a printed block start; the gap's size
        lines.append(line12(k=k, start=7, sizes=(1, 2, 3), starts=(0, v + 1, v + 5)))  # the second gap's start from the first
        lines.append(line12(k=k, start=0, sizes=(v, 3), starts=(0, v + 2), thick=(v, v + 1)))   # the thick pair
        lines.append(line12(k=k, start=0, sizes=(v, 3), starts=(0, v + 2), thick=(max(v - 1, 0), v)))
        k += 1
    lines.append(line12(k=k, start=TOP - 10, sizes=(3, 3), starts=(0, 7), thick=(TOP, TOP)))   # up to the largest plain coordinate
    lines.append(line12(k=k, start=TOP - 10, sizes=(10,), starts=(0,), thick=(TOP - 1, TOP)))
    lines.append("chr1\t%d\t%d" % (TOP - 1, TOP))
    got = check(engine, op, [bc.text_of(lines)])
    if op["kind"] not in ("n", "diff"):
        assert str(TOP).encode() in got[0][1]


@every_op
def test_short_and_long_labels_names_and_colours(engine, limits, op):
    T, S, _ = limits
    short = [line12("l", "c", "0", k) for k in range(T + 3)]
    room = 5000 if op["kind"] == "split" else S - len(br.run(op, bc.text_of(short[:T]))[0]) - 64   # what one line of tile 0 may add and the run still fit
    long_label = [line12("L" * (room - 1), "c", "0", 0)] + short[1:]
    long_name = short[:5] + [line12("l", "N" * (room - 1), "0", 5)] + short[6:]
    long_rgb = short[:9] + [line12("l", "c", "1" * (room - 1), 9)] + short[10:]
    every = short[:T - 1] + [line12("L" * (room // 3), "N" * (room // 3), "2" * (room // 3 - 2), T - 1)] + short[T:]
    check(engine, op, [bc.text_of(b) for b in (short, long_label, long_name, long_rgb, every)])


def test_split_runs_longer_than_its_stage_are_stored_by_their_lanes(engine, limits):
    """a label of 5000 bytes on every line: 256 printed lines are 1.3 MB, which no stage holds"""
    op = br.make_op("split")
    lines = [line12("L" * 5000, "chr%d" % (k % 7), k=k, sizes=(3, 4, 5), starts=(0, 10, 20)) for k in range(200)] + ["chr1\t5\t9\t" + "M" * 40000]
    check(engine, op, [bc.text_of(lines)])


def tile_of_output(op, T, total):
    """T plain lines whose printed text is `total` bytes: the first line's label is as long as that takes"""
    rest = [line12("l%d" % k, "chr1", k=k) for k in range(1, T)]
    first = lambda n: line12("L" * n, "chr1", k=0, strand="+")
    have = len(br.run(op, bc.text_of([first(1)] + rest))[0])
    text = bc.text_of([first(1 + total - have)] + rest)
    assert len(br.run(op, text)[0]) == total
    return text


@one_line_op
def test_a_run_at_the_stage_limit(engine, limits, op):
    T, S, _ = limits
    rng = random.Random(47)
    small = bc.text_of([bc.plain(rng) for _ in range(T + 1)])
    check(engine, op, [tile_of_output(op, T, S - 1) + small, tile_of_output(op, T, S), tile_of_output(op, T, S) + small])
    over = engine.blocks_text([(tile_of_output(op, T, S + 1) + small).encode(), small.encode()], device_op(op))
    assert over[0] == (32, b"", 0, 0)                                     # needs_host, nothing handed over
    assert over[1][0] == 0 and over[1][1].decode() == br.run(op, small)[0]          # ... and the block behind it is rendered


@pytest.mark.parametrize("flags", range(16))
def test_select_with_every_flag_combination(engine, limits, flags):
    op = br.make_op("select", bool(flags & 1), bool(flags & 2), bool(flags & 4), bool(flags & 8))
    rng = random.Random(53)
    lines = []
    for strand in "+-":
        for n in (1, 2, 3, 5):
            sizes, starts = bc.blocks_of(rng, n)
            lines.append(line12("s%s%d" % ("p" if strand == "+" else "m", n), "chr5", sizes=sizes, starts=starts, strand=strand, start=1000 * n))
        lines.append("\t".join(["chr5", "10", "90", "six", "0", strand]))
    lines.append("chr5\t10\t90")
    check(engine, op, [bc.text_of(lines * 9)])                            # (90 lines: more than a tile)
    got = engine.blocks_text([bc.text_of(lines).encode()], device_op(op))[0]
    assert (got[1] == b"") == (flags == 0)


def test_diff_lines_tiles_and_blocks_that_print_nothing(engine, limits):
    T = limits[0]
    op = br.make_op("diff")
    gap = lambda k: line12("g%d" % k, "chr3", k=k)
    quiet = lambda k: [line12("t%d" % k, "chr3", k=k, sizes=(10, 20, 5), starts=(0, 10, 30)), line12("o%d" % k, "chr3", k=k, sizes=(9,), starts=(0,)), "chr3\t4\t8\tq%d" % k][k % 3]
    some = [gap(k) if k % 5 == 0 else quiet(k) for k in range(2 * T + 9)]
    tile = [gap(k) for k in range(T)] + [quiet(k) for k in range(T)] + [gap(k) for k in range(T + 2)]      # the middle tile prints nothing
    first = [quiet(k) for k in range(T)] + [gap(k) for k in range(3)]
    block = [quiet(k) for k in range(2 * T + 1)]
    got = check(engine, op, [bc.text_of(b) for b in (some, tile, first, block, some)])
    assert got[3][1:] == (b"", 0, 0) and got[1][2] == 2 * T + 2 and got[2][2] == 3


def test_split_lines_whose_outputs_straddle_emit_tiles(engine, limits):
    M = limits[2]
    rng = random.Random(59)
    op = br.make_op("split")
    singles = lambda n: [bc.plain_short(rng) for _ in range(n)]
    lines = (singles(100) + [bc.plain12(rng, 300, max_gap=40, max_size=50)]           # outputs 100 .. 399: one tile seam inside the line
             + singles(7) + [bc.plain12(rng, M, max_gap=40, max_size=50)]             # outputs 407 .. 1430: four tile seams inside it
             + [bc.plain12(rng, OUT_TILE, max_gap=40, max_size=50)]                   # a line of exactly a tile, off the seams
             + singles(OUT_TILE - 151) + [bc.plain12(rng, 2 * OUT_TILE, max_gap=40, max_size=50)] + singles(5))
    counts = [int(l.split("\t")[9]) if len(l.split("\t")) == 12 else 1 for l in lines]
    firsts = [sum(counts[:k]) for k in range(len(lines))]
    inside = [any(f < s < f + c for f, c in zip(firsts, counts)) for s in range(OUT_TILE, sum(counts), OUT_TILE)]
    assert sum(inside) >= 7 and any(f % OUT_TILE == 0 and c == 2 * OUT_TILE for f, c in zip(firsts, counts))   # seams inside lines, and one line that fills two tiles
    check(engine, op, [bc.text_of(lines), bc.text_of(lines[::-1])])


def test_the_sink_gets_pieces_that_end_at_a_lines_end(engine, limits):
    rng = random.Random(61)
    text = bc.text_of([bc.plain12(rng, 3) for _ in range(500)])
    try:
        for op in (br.make_op("split"), br.make_op("strand", strand_op="r")):
            want = br.run(op, text)[0]
            engine.set_lines_chunk(4096)
            got = engine.blocks_text([text.encode()], device_op(op))[0]
            assert got[0] == 0 and got[1].decode() == want and got[3] >= len(want) // 4096
            assert got[3] <= len(want) // 3000 + 2                        # ... and no piece is much shorter than it may be
    finally:
        engine.set_lines_chunk(DEFAULT_CHUNK)


ERROR_LINES = ["chr1\t100\t200\tu\t0\t+\t100\t200\t0\t2\t10,10\t50,0", "chr1\t100\t200\tv\t0\t+\t100\t200\t0\t2\t60,50\t0,50", "chr1\t7",
               "chr1\t100\t200\tw\t0\t+\t100\t200\t0\t2\t60,40\t0,60\textra", "chr1\t5\t9\tx\t0\t*"]
ODD = [(k, None) for k in bc.ODD_KINDS] + [("error", l) for l in ERROR_LINES]


@pytest.mark.parametrize("kind,line", ODD, ids=[k if l is None else "error%d" % ERROR_LINES.index(l) for k, l in ODD])
def test_one_odd_line_brings_back_its_block_alone(engine, limits, kind, line):
    T = limits[0]
    rng = random.Random(67)
    line = line or bc.odd(rng, kind)
    assert not br.is_plain(line)
    plain = [bc.text_of([bc.plain(rng) for _ in range(T + 5)]) for _ in range(3)]
    for op in (br.make_op("split"), br.make_op("diff"), br.make_op("strand", strand_op="r")):
        for at in (0, T, T + 4):
            rows = plain[1].split("\n")[:-1]
            blocks = [plain[0], bc.text_of(rows[:at] + [line] + rows[at + 1:]), plain[2]]
            got = engine.blocks_text([b.encode() for b in blocks], device_op(op))
            assert got[1][0] != 0 and got[1][1:] == (b"", 0, 0)
            for k in (0, 2):
                assert got[k][0] == 0 and got[k][1].decode() == br.run(op, plain[k])[0]


def device_cases():
    out = []
    for c in CASES:
        data = [l for l in c["input"] if not br.rr.is_header(l)]
        if c["code"] == 0 and data and all(br.is_plain(l) for l in data) and c["op"].get("op", "+") in ("+", "-", "r"):
            out.append((c, data))
    return out


@pytest.mark.parametrize("case,data", device_cases(), ids=[c["name"] for c, _ in device_cases()])
def test_manifest_plain_cases_on_the_device(engine, case, data):
    want = case["stdout"]
    for l in case["input"]:
        if br.rr.is_header(l):                                        # (header lines are the tool's to echo)
            want = want[len(l) + 1:]
    got = engine.blocks_text([bc.text_of(data).encode()], device_op(br.norm_op(case["op"])))
    assert got[0][0] == 0 and got[0][1].decode() == want and got[0][2] == want.count("\n")


def test_the_manifest_has_plain_cases_of_every_operation():
    assert {c["op"]["kind"] for c, _ in device_cases()} == set(br.KINDS)
    assert len(device_cases()) >= 30


def test_argument_errors(engine, limits):
    bed = b"chr1\t5\t9\n"
    for op in (gtx.BlocksOp.make(6), gtx.BlocksOp.make(-1), gtx.BlocksOp.make("select", 16), gtx.BlocksOp.make("select", -1), gtx.BlocksOp.make("strand", 0, 3),
               gtx.BlocksOp.make("strand", 0, -1), gtx.BlocksOp.make("split", 32), gtx.BlocksOp.make("n", 0, 7)):
        with pytest.raises(gtx.GtxError):
            engine.blocks_text([bed], op)
    for kind in br.KINDS:
        assert engine.blocks_text([b""], gtx.BlocksOp.make(kind, 1))[0] == (0, b"", 0, 0)   # an empty block gives zero bytes
    assert engine.blocks_text([bed], gtx.BlocksOp.make("n"))[0][:3] == (0, b"_\t4\n", 1)
    assert engine.blocks_text([b"chr1\t5\t9\nchr1\t5"], gtx.BlocksOp.make("n"))[0][0] != 0   # (a block that does not end in a newline is not taken)
