"""gtx_rewrite_text / gtx_rewrite_result (include/gtx.h; kernels csrc/gtx_rewrite.hip) through the C ABI against the restatement
(tests/regionops_restate.py), byte for byte: every operation over blocks whose line counts sit on the lane, wave and tile seams, the
kept patterns of fix and bounds, outputs longer and shorter than the input, runs that start at every residue mod 16 of the
output, a tile whose run just fits and just misses the stage, the canary behind the output, two blocks in flight, and odd lines.
The canary is a check of the ABI: gtx_rewrite_result copies exactly out_bytes into the caller's buffer, so it shows that the entry
writes nothing behind the text's 16-byte unit there; the device buffer the emit pass stores into is the library's own and is not seen.
Tile and stage come from gtx_rewrite_limits."""
import json
import os

import numpy as np
import pytest

import gtx
import regionops_restate as rr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "regionops_manifest.json")))["cases"]
GENOME = {"chr1": 200_000, "chr2": 150_000}
OPS = [{"kind": "shift", "a": 150, "b": -90}, {"kind": "shift", "a": -3000, "b": 25}, {"kind": "shift", "a": 10 ** 12, "b": -10 ** 15},
       {"kind": "shiftp", "a": -500, "b": 1200}, {"kind": "pos", "op": "1", "c": 50}, {"kind": "pos", "op": "2", "c": 50}, {"kind": "pos", "op": "5p", "c": 0},
       {"kind": "pos", "op": "3p", "c": 700}, {"kind": "pos", "op": "c", "c": 20}, {"kind": "center"}, {"kind": "fix"}, {"kind": "bounds", "genome": GENOME}]


def op_id(o):
    return "-".join(str(v) for v in o.values() if not isinstance(v, dict))


def device_op(op):
    k = op["kind"]
    if k in ("shift", "shiftp"):
        return gtx.RewriteOp.make(k, op["a"], op["b"])
    if k == "pos":
        return gtx.RewriteOp.make(k, op["c"], 0, pos_op=op["op"])
    return gtx.RewriteOp.make(k, genome=op.get("genome"))


def plain_lines(seed, n):
    """n plain lines of 3 to 6 columns on three chromosomes (chr3 is in no genome), some inverted, some at the chromosome ends"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        s = int(rng.integers(0, 210_000)); ln = int(rng.integers(-40, 3000))
        cols = ["chr%d" % rng.integers(1, 4), str(s), str(max(s + ln, 0)), "r%d" % k, str(int(rng.integers(-5, 1000))), "+-"[int(rng.integers(0, 2))]]
        out.append("\t".join(cols[:int(rng.integers(3, 7))]))
    assert all(rr.is_plain(l) for l in out)
    return "".join(l + "\n" for l in out)


def check(engine, op, blocks):
    """every block printed as the restatement prints it, nothing written behind the text's 16-byte unit"""
    got = engine.rewrite_text([b.encode() for b in blocks], device_op(op))
    assert len(got) == len(blocks)
    for b, (redo, text, n, untouched) in zip(blocks, got):
        want = rr.run_plain(op, b)
        assert redo == 0
        assert text.decode() == want
        assert n == want.count("\n")
        assert untouched
    return got


@pytest.fixture(scope="module")
def limits():
    tile, stage = gtx.rewrite_limits()
    assert tile >= 64 and tile % 64 == 0 and stage >= 16 * tile
    return tile, stage


@pytest.mark.parametrize("op", OPS, ids=op_id)
def test_every_operation_at_the_block_sizes(engine, limits, op):
    T, _ = limits
    sizes = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    check(engine, op, [plain_lines(100 + n, n) for n in sizes])         # (eight blocks, two in flight, fetched in order)


@pytest.mark.parametrize("case", [c for c in CASES if c["code"] == 0 and all(rr.is_plain(l) for l in c["input"])], ids=lambda c: c["name"])
def test_manifest_cases_on_the_device(engine, case):
    got = engine.rewrite_text(["".join(l + "\n" for l in case["input"]).encode()], device_op(case["op"]))
    assert got[0][0] == 0 and got[0][1].decode() == case["stdout"] and got[0][3]


@pytest.mark.parametrize("kind", ["fix", "bounds"])
def test_kept_patterns(engine, limits, kind):
    T, _ = limits
    op = {"kind": "fix"} if kind == "fix" else {"kind": "bounds", "genome": {"chr1": 1000}}
    keep, drop = ("chr1\t5\t9\tk\n", "chr1\t9\t5\td\n") if kind == "fix" else ("chr1\t5\t2000\tk\t1\t-\n", "chr9\t5\t9\td\t1\t-\n")
    all_t, none_t = keep * T, drop * T
    first_t, last_t = keep + drop * (T - 1), drop * (T - 1) + keep
    blocks = [all_t * 3, none_t * 3, first_t * 3, last_t * 3, all_t + none_t + all_t, first_t + none_t + last_t + keep, none_t + none_t + keep]
    got = check(engine, op, blocks)
    assert [g[2] for g in got] == [3 * T, 0, 3, 3, 2 * T, 3, 1]


def test_outputs_longer_and_shorter_than_the_input(engine, limits):
    T, _ = limits
    grow = "".join("chr1\t%d\t%d\tg\n" % (9, 99) for _ in range(T + 3))
    shrink = "".join("chr1\t%d\t%d\ts\n" % (1000000000 + k, 1000000005 + k) for k in range(T + 3))
    got = check(engine, {"kind": "shift", "a": 10 ** 17, "b": 10 ** 18}, [grow])
    assert len(got[0][1]) > len(grow) + 30 * T
    got = check(engine, {"kind": "shift", "a": -10 ** 18, "b": -10 ** 18}, [grow])        # negative numbers: a sign and 18 digits
    assert got[0][1].count(b"-") == 2 * (T + 3)
    got = check(engine, {"kind": "shift", "a": -999999990, "b": -999999990}, [shrink])
    assert len(got[0][1]) <= len(shrink) - 14 * (T + 3)                    # both numbers go from 10 digits to at most 3


def test_runs_start_at_every_residue_of_the_output(engine, limits):
    T, _ = limits
    drop, tail = "chr1\t9\t5\n", "".join("chr2\t%d\t%d\tt%d\t0\t+\n" % (k, k + 50, k) for k in range(T + 7))
    blocks = []
    for r in range(16):                                                  # tile 0 keeps one line of 6 + r bytes: tile 1's run starts there
        head = "c" * (r + 1) + "\t0\t1\n"
        assert len(head) == 6 + r
        blocks.append(head + drop * (T - 1) + tail)
    got = check(engine, {"kind": "fix"}, blocks)
    assert sorted(len(b.split("\n")[0]) + 1 for b in blocks) == list(range(6, 22))
    assert all(g[2] == T + 8 for g in got)


def tile_of_bytes(T, total):
    """T identity lines whose text is `total` bytes"""
    per = total // T
    lines = ["n" * (per - 5) + "\t0\t1\n"] * (T - 1)
    lines.append("n" * (total - per * (T - 1) - 5) + "\t0\t1\n")
    text = "".join(lines)
    assert len(text) == total and text.count("\n") == T
    return text


def test_a_run_at_the_stage_limit(engine, limits):
    T, S = limits
    small = "chr1\t5\t9\n" * (T + 1)
    same = {"kind": "shift", "a": 0, "b": 0}
    check(engine, same, [tile_of_bytes(T, S - 1) + small, tile_of_bytes(T, S - 1), tile_of_bytes(T, S) + small, tile_of_bytes(T, S)])
    over = engine.rewrite_text([(tile_of_bytes(T, S + 1) + small).encode(), small.encode()], device_op(same))
    assert over[0][:3] == (32, b"", 0) and over[0][3]                      # needs_host, nothing written
    assert over[1][0] == 0 and over[1][1].decode() == small               # ... and the block behind it is rewritten
    # the text fits and the run does not: every line grows
    grown = engine.rewrite_text([tile_of_bytes(T, S).encode()], device_op({"kind": "shift", "a": 10 ** 9, "b": 10 ** 9}))
    assert grown[0][:3] == (32, b"", 0) and grown[0][3]


@pytest.mark.parametrize("odd", ["chr1 5 9 x", "chr1\t05\t9", "chr1\t5\t9\tx\t1\t.", "chr1\t5\t9\tx\t1\t+\t7\t8", "chr1\t5\t9\r", "chr1\t5"])
def test_one_odd_line_sends_the_block_back(engine, limits, odd):
    T, _ = limits
    lines = plain_lines(7, 2 * T + 5).split("\n")[:-1]
    assert not rr.is_plain(odd)
    for at in (0, len(lines) // 2, len(lines) - 1):
        block = "".join(l + "\n" for l in lines[:at] + [odd] + lines[at + 1:])
        got = engine.rewrite_text([block.encode()], device_op({"kind": "shift", "a": 1, "b": 1}))
        assert got[0][0] != 0 and got[0][1] == b"" and got[0][2] == 0 and got[0][3]


def test_amounts_the_device_does_not_take(engine):
    for a, b in ((2 ** 62 + 1, 0), (0, -2 ** 62 - 1)):
        with pytest.raises(gtx.GtxError):
            engine.rewrite_text([b"chr1\t5\t9\n"], gtx.RewriteOp.make("shift", a, b))
    check(engine, {"kind": "shift", "a": 2 ** 62, "b": -2 ** 62}, ["chr1\t5\t9\n"])
    assert engine.rewrite_text([b""], gtx.RewriteOp.make("fix"))[0][:3] == (0, b"", 0)
