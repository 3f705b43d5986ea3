"""gtx_convert_text / gtx_convert_result (include/gtx.h; kernels csrc/gtx_convert.hip) through the C ABI against the restatement
(tests/convert_restate.py), byte for byte, for SAM -> bed, SAM -> reg, GFF -> bed, GFF -> reg and BED -> reg: blocks whose line
counts sit on the lane, wave and tile seams, runs that start at every residue mod 16 of the output, labels and names of one byte and
as long as the stage lets them be, the digit-count seams of both numbers, every strand bit pattern and plain CIGAR operation, SAM
lines up to the tokenizer's limit, -chr and colours, a tile whose run just fits and just misses the stage, the canary behind the
output (a check of the ABI, as in test_gpu_rewrite.py), one odd line in one of three blocks, the manifest's plain cases and the
argument errors.  Tile, stage and the longest colour come from gtx_convert_limits."""
import json
import os

import pytest

import convert_restate as cr
import gtx
from convert_cases import gff_line, plain_bed, plain_gff, plain_sam, sam_line

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "convert_manifest.json")))["cases"]
PAIRS = [("sam", "bed"), ("sam", "reg"), ("gff", "bed"), ("gff", "reg"), ("bed", "reg")]
FLAG = {"sam": gtx.TEXT_SAM, "gff": gtx.TEXT_GFF, "bed": 0}
PLAIN = {"sam": plain_sam, "gff": plain_gff, "bed": plain_bed}
TOP = 2 ** 31 - 3                                                     # the largest coordinate the tokenizer calls plain

pair = pytest.mark.parametrize("fmt,to", PAIRS, ids=["%s-%s" % p for p in PAIRS])


def text_of(lines):
    return "".join(l + "\n" for l in lines)


def device_op(op):
    return gtx.ConvertOp.make(op["to"], op.get("chr", False), op.get("color"))


def check(engine, fmt, op, blocks):
    """every block printed as the restatement prints it, nothing written behind the text's 16-byte unit"""
    for b in blocks:
        assert all(cr.is_plain(l, fmt) for l in b.split("\n")[:-1])
    got = engine.convert_text([b.encode() for b in blocks], device_op(op), FLAG[fmt])
    assert len(got) == len(blocks)
    for b, (redo, text, n, untouched) in zip(blocks, got):
        want, err, code = cr.run(op, b, fmt)
        assert (err, code) == ("", 0)
        assert redo == 0
        assert text.decode() == want
        assert n == b.count("\n")
        assert untouched
    return got


def line_with(fmt, label, name, k=0):
    """a plain line of the format with this label and chromosome name"""
    if fmt == "sam":
        return sam_line(label, 16 * (k & 1), name, 100 + k, "36M")
    if fmt == "gff":
        return gff_line(name, 100 + k, 150 + k, "+-"[k & 1], label)
    return "\t".join([name, str(100 + k), str(150 + k), label, "0", "+-"[k & 1]])


def line_at(fmt, start, stop, k=0):
    """a plain line of the format whose region is [start, stop] (start >= 0; for BED start >= 1)"""
    if fmt == "sam":
        return sam_line("q%d" % k, 0, "chr1", start, "%dM" % (stop - start + 1), "*")
    if fmt == "gff":
        return gff_line("chr1", start, stop, "+", "g%d" % k)
    return "chr1\t%d\t%d\tb%d" % (start - 1, stop, k)


@pytest.fixture(scope="module")
def limits():
    tile, stage, max_color = gtx.convert_limits()
    assert tile >= 64 and tile % 64 == 0 and stage >= 16 * tile and max_color >= 11
    return tile, stage, max_color


@pair
def test_block_sizes_two_in_flight(engine, limits, fmt, to):
    T = limits[0]
    sizes = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    check(engine, fmt, {"to": to}, [text_of(PLAIN[fmt](n, 100 + n)) for n in sizes])      # (eight blocks, two in flight, fetched in order)


@pair
def test_runs_start_at_every_residue_of_the_output(engine, limits, fmt, to):
    T = limits[0]
    rest = [line_with(fmt, "l%d" % k, "chr2", k) for k in range(1, T + 7)]
    blocks = [text_of([line_with(fmt, "L" * r, "chr2")] + rest) for r in range(1, 17)]     # tile 1's run starts behind tile 0's: 16 lengths in a row
    check(engine, fmt, {"to": to}, blocks)
    starts = {len(cr.run({"to": to}, text_of(b.split("\n")[:T]), fmt)[0]) % 16 for b in blocks}
    assert starts == set(range(16))


@pair
def test_short_and_long_labels_and_names(engine, limits, fmt, to):
    T, S, _ = limits
    short = [line_with(fmt, "l", "c", k) for k in range(T + 3)]
    room = S - len(cr.run({"to": to}, text_of(short[:T]), fmt)[0]) - 64                    # what one line of tile 0 may add and the run still fit
    long_label = [line_with(fmt, "L" * (room - 1), "c")] + short[1:]
    long_name = short[:5] + [line_with(fmt, "l", "N" * (room - 1), 5)] + short[6:]
    both = short[:T - 1] + [line_with(fmt, "L" * (room // 2), "N" * (room // 2 - 1), T - 1)] + short[T:]
    check(engine, fmt, {"to": to}, [text_of(b) for b in (short, long_label, long_name, both)])


@pair
def test_digit_count_seams_of_both_numbers(engine, limits, fmt, to):
    lo = 1 if fmt == "bed" else 0                                       # START - 1 = -1: a read with POS 0, a feature with column 4 = 0
    edges = sorted({lo, 1, 2} | {10 ** j + d for j in range(1, 10) for d in (-1, 0, 1)})
    lines, k = [], 0
    for s in edges:                                                    # START - 1 across each seam, with a STOP close by and one far off
        for e in (s, s + 1, s + 9, min(s + 99999, TOP)):
            lines.append(line_at(fmt, s, e, k)); k += 1
    for e in edges + [TOP - 1, TOP]:                                    # STOP across each seam, up to the largest plain coordinate
        for s in (max(e - 1, lo), max(e - 200, lo)):
            lines.append(line_at(fmt, s, e, k)); k += 1
    lines.append(line_at(fmt, TOP, TOP, k))
    got = check(engine, fmt, {"to": to}, [text_of(lines)])
    if fmt != "bed" and to == "bed":
        assert got[0][1].startswith(b"chr1\t-1\t0\t")
    assert str(TOP).encode() in got[0][1]


@pytest.mark.parametrize("to", ["bed", "reg"])
def test_sam_strand_bits_and_cigar_operations(engine, limits, to):
    lines = [sam_line("f%d" % f, f, "chr1", 1000 + f, "36M") for f in (0, 16, 83, 99, 147, 163, 2064)]
    for k, cigar in enumerate(["5S40M5S", "10M2I10M", "10M3D10M", "5H20M", "4M1P4M", "10X", "4M2-4M", "3S2M1I2M1D2X1H"]):
        lines.append(sam_line("c%d" % k, 16 * (k & 1), "chr2", 500 + k, cigar))
        lines.append(sam_line("n%d" % k, 16 * (k & 1), "chr2", 500 + k, cigar, "*"))
    lines += [sam_line("star", 0, "chr3", 77, "*", "ACGTACG"), sam_line("starstar", 16, "chr3", 78, "*", "*"), sam_line("tags", 0, "chr3", 79, "*", "ACGT", ("NM:i:0", "XX:Z:a b"))]
    got = check(engine, "sam", {"to": to}, [text_of(lines)])
    minus = got[0][1].count(b"\t-\n") if to == "bed" else got[0][1].count(b" - ")
    assert minus == 4 + 8 + 1


@pytest.mark.parametrize("size", [100, 300, 560])
@pytest.mark.parametrize("to", ["bed", "reg"])
def test_sam_lines_up_to_the_tokenizers_limit(engine, limits, to, size):
    T = limits[0]
    lines = []
    for k in range(T + 1):
        base = sam_line("read%04d" % k, 16 * (k % 2), "chr%d" % (k % 3 + 1), 10_000 + 37 * k, "20M")
        lines.append(base + "\tXX:Z:" + "x" * (size - len(base) - 7))
    assert {len(l) + 1 for l in lines} == {size}
    check(engine, "sam", {"to": to}, [text_of(lines)])


@pytest.mark.parametrize("fmt", ["sam", "gff"])
def test_ucsc_names_and_colours(engine, limits, fmt):
    T, _, M = limits
    names = ["MT", "1", "chrX", "M", "MTX", "T", "MT"]
    lines = [line_with(fmt, "l%d" % k, names[k % len(names)], k) for k in range(T + 9)]
    for op in ({"to": "bed", "chr": True}, {"to": "bed", "color": "7"}, {"to": "bed", "chr": True, "color": "c" * M}, {"to": "reg", "chr": True, "color": "9,9,9"}):
        got = check(engine, fmt, op, [text_of(lines)])
        if op.get("chr") and op["to"] == "bed":
            assert got[0][1].startswith(b"chrM\t") and b"\nchrMTX\t" in got[0][1] and b"\nchrchrX\t" in got[0][1]


def tile_of_output(fmt, op, T, total):
    """T plain lines whose printed text is `total` bytes: the first line's label is as long as that takes"""
    rest = [line_with(fmt, "l%d" % k, "chr1", k) for k in range(1, T)]
    have = len(cr.run(op, text_of([line_with(fmt, "L", "chr1")] + rest), fmt)[0])
    text = text_of([line_with(fmt, "L" * (1 + total - have), "chr1")] + rest)
    assert len(cr.run(op, text, fmt)[0]) == total
    return text


@pair
def test_a_run_at_the_stage_limit(engine, limits, fmt, to):
    T, S, _ = limits
    op = {"to": to}
    small = text_of(PLAIN[fmt](T + 1, 3))
    check(engine, fmt, op, [tile_of_output(fmt, op, T, S - 1) + small, tile_of_output(fmt, op, T, S), tile_of_output(fmt, op, T, S) + small])
    over = engine.convert_text([(tile_of_output(fmt, op, T, S + 1) + small).encode(), small.encode()], device_op(op), FLAG[fmt])
    assert over[0][:3] == (32, b"", 0) and over[0][3]                      # needs_host, nothing written
    assert over[1][0] == 0 and over[1][1].decode() == cr.run(op, small, fmt)[0]             # ... and the block behind it is converted


ODD = {
    "sam": [sam_line("sp", 0, "chr1", 100, "10M100N10M"), sam_line("eq", 0, "chr1", 100, "10=", "*"), sam_line("ten", 0, "chr1", 100, "10M").rsplit("\t", 1)[0],
            sam_line("cr", 0, "chr1", 100, "10M") + "\r", sam_line("two words", 0, "chr1", 100, "10M")],
    "gff": [gff_line("chr1", 5, 9, ".", "l"), gff_line("chr1", 5, 9, "+", "l", "c") + "\textra"],
    "bed": ["chr1 5 9 l", "chr1\t5\t9\tl\t0\t.", "chr1\t5\t9\tl\t0\t+\t7"],
}


@pytest.mark.parametrize("fmt,to,odd", [(f, t, o) for f, t in PAIRS for o in range(len(ODD[f]))], ids=lambda v: str(v))
def test_one_odd_line_brings_back_its_block_alone(engine, limits, fmt, to, odd):
    T = limits[0]
    line = ODD[fmt][odd]
    assert not cr.is_plain(line, fmt)
    plain = [text_of(PLAIN[fmt](T + 5, 20 + k)) for k in range(3)]
    for at in (0, T, T + 4):
        rows = plain[1].split("\n")[:-1]
        blocks = [plain[0], text_of(rows[:at] + [line] + rows[at + 1:]), plain[2]]
        got = engine.convert_text([b.encode() for b in blocks], device_op({"to": to}), FLAG[fmt])
        assert got[1][0] != 0 and got[1][1:] == (b"", 0, True)
        for k in (0, 2):
            assert got[k][0] == 0 and got[k][1].decode() == cr.run({"to": to}, plain[k], fmt)[0] and got[k][3]


def device_cases():
    out = []
    for c in CASES:
        data = [l for l in c["input"] if not cr.is_header(l, c["fmt"])]
        if c["code"] == 0 and data and all(cr.is_plain(l, c["fmt"]) for l in data) and not c["op"].get("title") and not c["op"].get("position"):
            out.append((c, data))
    return out


@pytest.mark.parametrize("case,data", device_cases(), ids=[c["name"] for c, _ in device_cases()])
def test_manifest_plain_cases_on_the_device(engine, case, data):
    got = engine.convert_text([text_of(data).encode()], device_op(case["op"]), FLAG[case["fmt"]])
    assert got[0][0] == 0 and got[0][1].decode() == case["stdout"] and got[0][2] == len(data) and got[0][3]


def test_the_manifest_has_plain_cases_of_every_pair():
    assert {(c["fmt"], c["op"]["to"]) for c, _ in device_cases()} == set(PAIRS)


def test_argument_errors(engine, limits):
    M = limits[2]
    sam, bed = sam_line("q", 0, "chr1", 5, "10M").encode() + b"\n", b"chr1\t5\t9\n"
    bad = [(bed, gtx.ConvertOp.make("bed"), 0),                                             # BED text into BED lines
           (sam, gtx.ConvertOp.make("bed"), gtx.TEXT_SAM | gtx.TEXT_GFF),                   # both format flags
           (sam, gtx.ConvertOp.make(2), gtx.TEXT_SAM), (sam, gtx.ConvertOp.make(-1), gtx.TEXT_SAM),   # an unknown target
           (sam, gtx.ConvertOp.make("bed", color="c" * (M + 1)), gtx.TEXT_SAM),            # a colour beyond max_color
           (sam, gtx.ConvertOp.make("bed"), gtx.TEXT_SAM | 1)]                              # a flag that is no format
    for text, op, flags in bad:
        with pytest.raises(gtx.GtxError):
            engine.convert_text([text], op, flags)
    assert engine.convert_text([b""], gtx.ConvertOp.make("reg"), 0)[0][:3] == (0, b"", 0)
    got = engine.convert_text([sam], gtx.ConvertOp.make("bed", color="c" * M), gtx.TEXT_SAM)
    assert got[0][0] == 0 and got[0][1] == b"chr1\t4\t14\tq\t1000\t+\t4\t14\t" + b"c" * M + b"\n"
