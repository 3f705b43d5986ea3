"""genomic_subset (csrc/genomic_subset.cpp, GtxPrintSubset in csrc/gtx_host_join.cpp): the test regions that overlap some
reference region, with -inv those that overlap none.  Expected output: the query lines whose count in the oracle's `qstats`
(oracle/gtx_oracle.c: the reference's CountQueryOverlaps per query line) is > 0 (== 0 with -inv), each rendered through a
restatement of GenomicRegionBED::Read and ::Print (genomic_intervals.cpp:2157-2218) below, the file's header lines first; errors:
the oracle's exit code and message, with the lines selected before the error on stdout.  Every run is made three ways -- the
loop alone (GTX_TEXT_ON_DEVICE=0), the text path, and the text path over blocks of 1 MB -- and GTX_TEXT_TRACE's line must say which
way it went: a run may not pass by quietly taking the other path.  The merge's stop (Done(), which the oracle does not model) is
held to hand-derived vectors (tests/golden/subset_manifest.json) and to the reference's subset loop on the class layer
(tests/tools/subset_caller.cpp)."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import orc
from oracle.restate import NAMES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
TOOL = os.path.join(CSRC, "genomic_subset")
CALLER = os.path.join(CSRC, "subset_caller")
GOLD = os.path.join(ROOT, "tests", "golden")

WAYS = [("loop", {"GTX_TEXT_ON_DEVICE": "0"}), ("text", {"GTX_TEXT_ON_DEVICE": "1"}),
        ("blocks", {"GTX_TEXT_ON_DEVICE": "1", "GTX_PACK_BLOCK_MB": "1"})]
TRACE = re.compile(r"^\[gtx subset\] blocks selected on the device: (\d+), (?:none came back|the loop took over at block (\d+) \(line (\d+)\))\n", re.M)


def tool(args, cwd, env=None, stdin=None):
    e = dict(os.environ, GTX_TEXT_TRACE="1")
    for k in ("GTX_TEXT_ON_DEVICE", "GTX_PACK_BLOCK_MB"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([TOOL] + args, capture_output=True, cwd=cwd, env=e, input=stdin)
    err = r.stderr.decode()
    m = TRACE.search(err)
    trace = None if m is None else dict(on_device=int(m.group(1)), block=None if m.group(2) is None else int(m.group(2)),
                                        line=None if m.group(3) is None else int(m.group(3)))
    return r.returncode, r.stdout.decode(), TRACE.sub("", err), trace


# ---- the reference, restated: GenomicRegionBED::Read (tokens as CountTokens / GetNextToken cut them, core.cpp:577-625) and ::Print ----

def atol(t):
    m = re.match(r"[ \t\n\v\f\r]*([+-]?\d+)", t)
    return int(m.group(1)) if m else 0


def count_tokens(s, d):
    k = 0
    while k < len(s) and s[k] == " ":
        k += 1
    n = 0
    while k < len(s):
        while k < len(s) and s[k] != d:
            k += 1
        if k < len(s):
            k += 1
        n += 1
        while k < len(s) and s[k] == " ":
            k += 1
    return n


def next_token(s, k, d):
    while k < len(s) and s[k] == " ":
        k += 1
    e = s.find(d, k)
    return (s[k:], len(s)) if e < 0 else (s[k:e], e + 1)


def render(line):
    """what Print writes for the region Read makes of the line"""
    d = "\t" if "\t" in line else " "
    n = count_tokens(line, d)
    tok, k = [], 0
    for _ in range(n):
        t, k = next_token(line, k, d)
        tok.append(t)
    start = atol(tok[1]) + 1
    iv = [(start, atol(tok[2]))]
    if n == 12:
        cnt = atol(tok[9])
        sizes = [atol(x) for x in tok[10].split(",")] + [0] * cnt
        starts = [atol(x) for x in tok[11].split(",")] + [0] * cnt
        iv = [(start + starts[j], start + starts[j] + sizes[j] - 1) for j in range(cnt)]
    s = "%s\t%d\t%d" % (tok[0], iv[0][0] - 1, iv[-1][1])
    if n >= 4:
        s += "\t" + tok[3]
        if n >= 5:
            s += "\t%d" % atol(tok[4])
            if n >= 6:
                s += "\t" + ("-" if tok[5] in ("-", "-1") else "+")
                if n >= 8:
                    s += "\t%d\t%d" % (atol(tok[6]), atol(tok[7]))
                    if n >= 9:
                        s += "\t" + tok[8]
                        if n == 12:
                            s += "\t%d\t%s\t0%s" % (len(iv), ",".join(str(b - a + 1) for a, b in iv), "".join(",%d" % (a - iv[0][0]) for a, _ in iv[1:]))
    return s + "\n"


def is_header(line):
    return line.startswith("track ") or line.startswith("browser ")


def oracle(opts, ref, qry, cwd):
    """(exit code, stderr, {query line number: count}) of qstats; -inv is not the oracle's business"""
    o = subprocess.run([orc.CLI, "qstats"] + [x for x in opts if x != "-inv"] + [ref, qry], capture_output=True, cwd=cwd)
    rows = [r.split("\t") for r in o.stdout.decode().splitlines()]
    return o.returncode, o.stderr.decode(), {int(r[0]): int(r[1]) for r in rows}


def expected(opts, lines, counts):
    """header lines, then the lines the oracle got to and selected, rendered; and the selected share"""
    inv = "-inv" in opts
    out, n_sel = "", 0
    k = 0
    while k < len(lines) and is_header(lines[k]):
        out += lines[k] + "\n"
        k += 1
    for no in sorted(counts):
        if (counts[no] == 0) == inv:
            out += render(lines[no - 1]); n_sel += 1
    return out, n_sel / max(len(counts), 1)


# ---- inputs ----

def bed_lines(rng, n, span, lmax, cols=6, sort="pos", multi=0.0, prefix="q"):
    """test_gpu_join_cli.py's generator: three chromosomes, random strands, scores that print as they stand"""
    rows = []
    for i in range(n):
        c = int(rng.integers(0, 3)); s = int(rng.integers(0, span)); st = "+-"[int(rng.integers(0, 2))]
        if cols == 12 and rng.random() < multi:
            at, iv = s, []
            for _ in range(int(rng.integers(2, 5))):
                sz = int(rng.integers(5, 60)); iv.append((at, at + sz)); at += sz + int(rng.integers(20, 400))
        else:
            iv = [(s, s + int(rng.integers(1, lmax)))]
        rows.append((c, iv[0][0], st, iv))
    if sort == "pos":
        rows.sort(key=lambda r: (r[0], r[1]))
    elif sort == "strand":
        rows.sort(key=lambda r: (r[0], r[2], r[1]))
    out = []
    for i, (c, s, st, iv) in enumerate(rows):
        e = iv[-1][1]
        cols_ = [NAMES[c], str(s), str(e), "%s%d" % (prefix, i), str(int(rng.integers(0, 1000)) * (-1 if i % 17 == 0 else 1)), st]
        if cols == 12:
            cols_ += [str(s + 1), str(e - 1), "255,0,0", str(len(iv)), ",".join(str(b - a) for a, b in iv) + ",", ",".join(str(a - s) for a, _ in iv) + ","]
        out.append("\t".join(cols_[:cols]))
    return out


def write(path, lines):
    path.write_text("".join(l + "\n" for l in lines))


N_REF, N_QRY, SPAN, LMAX = 1500, 100_000, 400_000, 400      # 2 to 4 MB of query text: several blocks of 1 MB


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("subsetcli")
    rng = np.random.default_rng(99)
    write(d / "refs.bed", bed_lines(rng, N_REF, SPAN, LMAX, prefix="r"))
    write(d / "refs_s.bed", bed_lines(rng, N_REF, SPAN, LMAX, sort="strand", prefix="r"))
    write(d / "refs12.bed", bed_lines(rng, N_REF, SPAN, LMAX, cols=12, multi=0.5, prefix="r"))
    for cols in (3, 4, 5, 6):
        write(d / ("q%d.bed" % cols), bed_lines(rng, N_QRY, SPAN, LMAX, cols=cols))
    write(d / "q_s.bed", bed_lines(rng, N_QRY, SPAN, LMAX, sort="strand"))
    write(d / "q12.bed", bed_lines(rng, 30_000, SPAN, LMAX, cols=12, multi=0.3))
    write(d / "qshuf.bed", bed_lines(rng, N_QRY, SPAN, LMAX, sort="none"))
    write(d / "qhead.bed", ["track name=reads", "browser position chr1:1-100"] + bed_lines(rng, N_QRY, SPAN, LMAX))
    with gzip.open(d / "q6.bed.gz", "wt") as f:
        f.write((d / "q6.bed").read_text())
    return d


def three_ways(files, opts, ref, qry, device=True, share=True):
    """the run made three ways; every output is the oracle's, and the trace says the text path took all blocks (device) or gave
    the file to the loop at its first block (not device)"""
    rc_o, err_o, counts = oracle(opts, ref, qry, files)
    assert rc_o == 0, err_o
    lines = (files / qry).read_text().split("\n")[:-1]
    want, sel = expected(opts, lines, counts)
    if share:
        assert 0.1 <= sel <= 0.9, sel                                         # not by selecting nothing, or everything
    outs = []
    for name, env in WAYS:
        rc, out, err, trace = tool(opts + [ref, qry], files, env)
        assert (rc, err) == (0, ""), (name, err)
        assert out == want, name
        outs.append(out)
        if name == "loop":
            assert trace is None
        elif device:
            assert trace is not None and trace["block"] is None, (name, trace)
            assert trace["on_device"] == 1 if name == "text" else trace["on_device"] >= 2, (name, trace)
        else:
            assert trace is not None and trace["block"] == 1 and trace["on_device"] == 0, (name, trace)
    assert outs[0] == outs[1] == outs[2]
    return sel


MAIN = [([], "refs.bed", "q6.bed"), (["-i"], "refs.bed", "q6.bed"), (["-S"], "refs.bed", "q6.bed"), (["-S", "-i"], "refs.bed", "q6.bed"),
        (["-S", "-s"], "refs_s.bed", "q_s.bed")]


@pytest.mark.parametrize("inv", [[], ["-inv"]], ids=["plain", "inv"])
@pytest.mark.parametrize("opts,ref,qry", MAIN, ids=[" ".join(r[0]) or "none" for r in MAIN])
def test_cli_equals_the_restated_reference(files, opts, ref, qry, inv):
    three_ways(files, opts + inv, ref, qry)


@pytest.mark.parametrize("cols", [3, 4, 5])
def test_fewer_columns(files, cols):
    three_ways(files, ["-i"], "refs.bed", "q%d.bed" % cols)
    three_ways(files, ["-S", "-inv"], "refs.bed", "q%d.bed" % cols)


def test_the_selected_shares_are_the_ones_the_fixture_was_sized_for(files):
    """1500 reference lines of up to 400 bases on three chromosomes of 400 000: about a fifth of the queries overlap one on their
    strand, two fifths on either"""
    aware = three_ways(files, [], "refs.bed", "q6.bed")
    either = three_ways(files, ["-i"], "refs.bed", "q6.bed")
    assert 0.15 < aware < 0.30 and 0.30 < either < 0.50


def test_shuffled_queries_and_bin_bits(files):
    three_ways(files, ["-i"], "refs.bed", "qshuf.bed")
    three_ways(files, ["-B", "10,14,18"], "refs.bed", "q6.bed")
    three_ways(files, ["-i", "-inv", "-B", "10,14,18"], "refs.bed", "qshuf.bed")


@pytest.mark.parametrize("opts", [["-i"], ["-i", "-gaps"], ["-S", "-i"], ["-S", "-gaps", "-inv"], ["-inv"]], ids=lambda o: " ".join(o))
def test_bed12_on_either_side(files, opts):
    """12-column queries are printed through Print's own columns 10-12: every block of them goes back to the loop"""
    three_ways(files, opts, "refs12.bed", "q12.bed", device=False)
    three_ways(files, opts, "refs12.bed", "q6.bed")                            # single-interval queries over regions with blocks: the text path takes them


def test_header_lines_are_echoed_first(files):
    three_ways(files, ["-i"], "refs.bed", "qhead.bed")
    three_ways(files, ["-S", "-inv"], "refs.bed", "qhead.bed")
    assert tool(["-i", "refs.bed", "qhead.bed"], files, WAYS[1][1])[1].startswith("track name=reads\nbrowser position chr1:1-100\nchr")


def test_stdin_and_gz_take_the_loop(files):
    for opts in (["-i"], ["-S", "-inv"]):
        rc_o, _, counts = oracle(opts, "refs.bed", "q6.bed", files)
        want, _ = expected(opts, (files / "q6.bed").read_text().split("\n")[:-1], counts)
        for _, env in WAYS:
            rc, out, err, trace = tool(opts + ["refs.bed"], files, env, stdin=(files / "q6.bed").read_bytes())
            assert (rc, out, err, trace) == (0, want, "", None)
            rc, out, err, trace = tool(opts + ["refs.bed", "q6.bed.gz"], files, env)
            assert (rc, out, err, trace) == (0, want, "", None)


# ---- lines that send their block back: one kind per run, once in the first block and once in a later one ----

def odd_line(kind, line):
    c, s, e, lab, sc, st = line.split("\t")
    return {
        "space-separated": " ".join([c, s, e, lab, sc, st]),
        "leading-zero": "\t".join([c, "00" + s, e]),
        "plus-sign": "\t".join([c, "+" + s, e, lab]),
        "strand-dot": "\t".join([c, s, e, lab, sc, "."]),
        "strand-1": "\t".join([c, s, e, lab, sc, "1"]),
        "score-1.5": "\t".join([c, s, e, lab, "1.5", st]),
        "score-007": "\t".join([c, s, e, lab, "007", st]),
        "seven-columns": "\t".join([c, s, e, lab, sc, st, "0"]),
        "bed12": "\t".join([c, s, str(int(s) + 300), lab, sc, st, s, e, "0", "2", "50,100,", "0,200,"]),
        "crlf": "\t".join([c, s, e]) + "\r",
        "empty-label": "\t".join([c, s, e, "", sc, st]),
    }[kind]


KINDS = ["space-separated", "leading-zero", "plus-sign", "strand-dot", "strand-1", "score-1.5", "score-007", "seven-columns", "bed12", "crlf",
         "empty-label"]


@pytest.mark.parametrize("opts", [["-i"], ["-S", "-i"]], ids=["bin", "merge"])
@pytest.mark.parametrize("where", ["first-block", "later-block"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_line_the_device_does_not_take_sends_its_block_back(files, kind, where, opts):
    lines = (files / "q6.bed").read_text().split("\n")[:-1]
    at = 40 if where == "first-block" else (len(lines) * 4) // 5
    lines[at] = odd_line(kind, lines[at])
    if kind == "plus-sign" and lines[at].split("\t")[1] == "+0":
        pytest.fail("the fixture's line starts at 0: +0 is still a sign, but pick another seed")
    name = "odd.bed"
    write(files / name, lines)
    assert render(lines[at]) != lines[at] + "\n" or kind == "empty-label"     # (an empty label prints as it stands: the tokenizer is what refuses it)
    rc_o, err_o, counts = oracle(opts, "refs.bed", name, files)
    assert rc_o == 0, err_o
    for inv in ([["-inv"]] if "-S" in opts else [[]]):                          # (both senses, one per algorithm)
        want, _ = expected(opts + inv, lines, counts)
        assert (render(lines[at]) in want) == ((counts[at + 1] == 0) == bool(inv))
        outs = []
        for wname, env in WAYS:
            rc, out, err, trace = tool(opts + inv + ["refs.bed", name], files, env)
            assert (rc, err) == (0, ""), (wname, err)
            assert out == want, wname
            outs.append(out)
            if wname == "loop":
                assert trace is None
                continue
            assert trace is not None and trace["block"] is not None, (wname, trace)        # the loop took over ...
            if wname == "text" or where == "first-block":                               # ... at the one block, or the first
                assert trace["block"] == 1 and trace["line"] == 2 and trace["on_device"] == 0, (wname, trace)
            else:                                                                        # ... at the block that holds the line, not before
                assert trace["block"] >= 3 and trace["on_device"] == trace["block"] - 1, (wname, trace)
                assert trace["line"] <= at + 1 and sum(len(l) + 1 for l in lines[trace["line"] - 1:at + 1]) <= (1 << 20), (wname, trace)
        assert outs[0] == outs[1] == outs[2]


def text_blocks(data, block_bytes=1 << 20):
    """[first line, last line] (1-based) of the blocks the text path reads: the set's constructor takes line 1, then up to
    block_bytes at a time, cut behind the last complete line (LineSource::ReadTextInto)"""
    pos, line, out = data.index(b"\n") + 1, 2, []
    while pos < len(data):
        keep = data[pos:pos + block_bytes].rindex(b"\n") + 1
        n = data.count(b"\n", pos, pos + keep)
        out.append((line, line + n - 1))
        pos += keep; line += n
    return out


COUNT_TRACE = re.compile(r"^\[gtx text\] blocks tokenised on the device: (\d+), sent back to the host packer: (\d+), packed on the host from the start: (\d+)\n", re.M)


def test_a_refusal_in_the_second_of_two_blocks_in_flight(tmp_path):
    """Three blocks of 1 MB, the one line the device does not take in the middle of block 2: its verdict comes in while block 3 is in
    flight.  The two users of the text pump part ways there: genomic_overlaps count packs block 2 on the host and keeps block 3's
    counts from the device; genomic_subset hands the file to the loop from block 2's first line on and drops what block 3 selected."""
    rng = np.random.default_rng(7)
    write(tmp_path / "refs.bed", bed_lines(rng, N_REF, SPAN, LMAX, prefix="r"))
    lines = bed_lines(rng, 80_000, SPAN, LMAX)
    blocks = text_blocks("".join(l + "\n" for l in lines).encode())
    assert len(blocks) == 3, blocks
    at = (blocks[1][0] + blocks[1][1]) // 2                                      # (file line, 1-based)
    lines[at - 1] = odd_line("plus-sign", lines[at - 1])                        # (a sign: neither tokenizer takes it; a leading zero the count path does)
    assert not lines[at - 1].split("\t")[1].startswith("+0")
    write(tmp_path / "odd.bed", lines)
    blocks = text_blocks((tmp_path / "odd.bed").read_bytes())                    # (the line is shorter now)
    assert len(blocks) == 3 and blocks[1][0] + 100 < at < blocks[1][1] - 100, blocks   # in block 2, off its seams

    def count(env):
        e = dict(os.environ, GTX_TEXT_TRACE="1", **env)
        r = subprocess.run([os.path.join(CSRC, "genomic_overlaps"), "count", "-i", "refs.bed", "odd.bed"], capture_output=True, cwd=tmp_path, env=e)
        err = r.stderr.decode()
        m = COUNT_TRACE.search(err)
        return r.returncode, r.stdout, COUNT_TRACE.sub("", err), None if m is None else tuple(int(g) for g in m.groups())

    rc0, out0, err0, trace0 = count({"GTX_TEXT_ON_DEVICE": "0"})
    rc1, out1, err1, trace1 = count(WAYS[2][1])
    assert (rc0, err0, trace0) == (0, "", None) and len(out0) > 0
    assert (rc1, err1, trace1) == (0, "", (2, 1, 0))
    assert out1 == out0

    rc0, out0, err0, trace0 = tool(["-i", "refs.bed", "odd.bed"], tmp_path, WAYS[0][1])
    rc1, out1, err1, trace1 = tool(["-i", "refs.bed", "odd.bed"], tmp_path, WAYS[2][1])
    assert (rc0, err0, trace0) == (0, "", None) and 0.1 < out0.count("\n") / len(lines) < 0.9
    assert (rc1, err1) == (0, "") and trace1 == dict(on_device=1, block=2, line=blocks[1][0])
    assert out1 == out0


# ---- errors: exit 1, the reference's message and line number, the lines selected before it on stdout ----

def with_error(kind, refs, lines):
    at = len(lines) // 2
    if kind == "zero-length-read":
        c, s, e, lab, sc, st = lines[at].split("\t")
        lines[at] = "\t".join([c, s, s, lab, sc, st])
        return [], refs, lines
    if kind == "query-out-of-order":
        lines[at], lines[at + 300] = lines[at + 300], lines[at]
        return ["-S"], refs, lines
    if kind == "index-out-of-order":
        k = len(refs) // 2
        refs[k], refs[k + 40] = refs[k + 40], refs[k]
        return ["-S"], refs, lines
    if kind == "malformed-line":
        lines[at] = "\t".join(lines[at].split("\t")[:2])
        return [], refs, lines
    if kind == "malformed-line-merge":
        lines[at] = "\t".join(lines[at].split("\t")[:2])
        return ["-S"], refs, lines
    raise AssertionError(kind)


@pytest.mark.parametrize("inv", [[], ["-inv"]], ids=["plain", "inv"])
@pytest.mark.parametrize("kind", ["zero-length-read", "query-out-of-order", "index-out-of-order", "malformed-line", "malformed-line-merge"])
def test_errors_after_the_lines_before_them(files, kind, inv):
    refs = (files / "refs.bed").read_text().split("\n")[:-1]
    lines = (files / "q6.bed").read_text().split("\n")[:-1]
    opts, refs, lines = with_error(kind, refs, lines)
    write(files / "erefs.bed", refs); write(files / "equery.bed", lines)
    opts = opts + ["-i"] + inv
    rc_o, err_o, counts = oracle(opts, "erefs.bed", "equery.bed", files)
    assert rc_o == 1 and 1000 < len(counts) < len(lines)
    want, _ = expected(opts, lines, counts)
    for name, env in WAYS:
        rc, out, err, trace = tool(opts + ["erefs.bed", "equery.bed"], files, env)
        assert rc == 1 and err.strip() == err_o.strip(), (name, err)
        assert out == want, name
        if name == "blocks" and kind != "index-out-of-order":                  # (an index set out of order is the loop's from the start)
            assert trace is not None and trace["block"] >= 2, trace


TOO_BIG = "coordinate does not fit the packed 32-bit representation of the MI355X path!"


@pytest.mark.parametrize("opts", [["-i"], ["-S", "-i", "-inv"]], ids=lambda o: " ".join(o))
def test_a_coordinate_beyond_32_bits_is_the_loops_error(files, opts):
    """the packed triples hold 32-bit coordinates: a line beyond them is no plain line for the device, its block comes back, and the
    loop ends there with the project's message, after the lines selected before it"""
    lines = (files / "q6.bed").read_text().split("\n")[:-1]
    at = (len(lines) * 4) // 5 if "-S" not in opts else len(lines)              # (under -S behind everything: the order holds)
    lines.insert(at, "chr3\t3000000000\t3000000050\tbig\t0\t+")
    write(files / "big.bed", lines); write(files / "before.bed", lines[:at])
    rc_o, err_o, counts = oracle(opts, "refs.bed", "before.bed", files)
    assert rc_o == 0 and len(counts) == at
    want, _ = expected(opts, lines, counts)
    for name, env in WAYS:
        rc, out, err, trace = tool(opts + ["refs.bed", "big.bed"], files, env)
        assert (rc, err.strip()) == (1, "Error: Line %d: %s" % (at + 1, TOO_BIG)), (name, err)
        assert out == want, name
        if name == "blocks":
            assert trace is not None and trace["block"] >= 3 and trace["line"] <= at + 1, trace


# ---- the stop: under -S the loop ends at Done() unless -inv ----

STOPS = json.load(open(os.path.join(GOLD, "subset_manifest.json")))["cases"]


@pytest.mark.parametrize("case", STOPS, ids=[c["name"] for c in STOPS])
def test_hand_derived_stop_vectors(case):
    for name, env in WAYS:
        rc, out, err, _ = tool(case["args"], GOLD, env)
        assert (rc, out, err.strip()) == (case["rc"], case["stdout"], case["stderr"]), name


LATE = [("s1_reads_late_unsorted.bed", "query regions are not sorted (sorted-by-strand = false)!"),
        ("s1_reads_late_malformed.bed", "number of tokens should be at least 3 for BED format!")]


@pytest.mark.parametrize("golden,what", LATE, ids=["order-violation", "malformed-line"])
def test_the_stop_with_the_offending_line_in_a_later_block(tmp_path, golden, what):
    """the golden vectors with 60 000 queries behind the stop in front of the offending line: over blocks of 1 MB the line
    lies blocks behind the stop.  Without -inv nothing behind q2 overlaps, the block with the line comes back, and the loop, reading
    the file again, ends at Done() before it gets there: exit 0.  With -inv every query behind q2 is printed, then the error"""
    refs = open(os.path.join(GOLD, "s1_refs.bed")).read()
    q = open(os.path.join(GOLD, golden)).read().split("\n")[:-1]
    fill = ["chr1\t%d\t%d\tf%d\t0\t-" % (1000 + 7 * i, 1100 + 7 * i, i) for i in range(60_000)]
    lines = q[:4] + fill + q[4:]
    (tmp_path / "r.bed").write_text(refs); write(tmp_path / "q.bed", lines)
    assert sum(len(l) + 1 for l in lines) > (1 << 20)
    msg = "Error: Line %d: %s" % (len(fill) + 5, what)
    for name, env in WAYS:
        rc, out, err, trace = tool(["-S", "-i", "r.bed", "q.bed"], tmp_path, env)
        assert (rc, out, err) == (0, "".join(l + "\n" for l in q[:2]), ""), name
        if name == "blocks":
            assert trace["block"] >= 2 and trace["on_device"] == trace["block"] - 1, trace
        rc, out, err, trace = tool(["-S", "-i", "-inv", "r.bed", "q.bed"], tmp_path, env)
        assert (rc, out, err.strip()) == (1, "".join(l + "\n" for l in q[2:4] + fill), msg), name


def caller(args, cwd):
    r = subprocess.run([CALLER] + args, capture_output=True, cwd=cwd, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def blur(rng, lines, zero, inverted):
    """a share of the lines made zero-length (BED start == end) / inverted (start > end): the merge takes both"""
    out = []
    for l in lines:
        t = l.split("\t")
        u = rng.random()
        if u < zero:
            t[2] = t[1]
        elif u < zero + inverted:
            t[2] = str(max(0, int(t[1]) - int(rng.integers(1, 40))))
        out.append("\t".join(t))
    return out


@pytest.mark.parametrize("tail", ["order-violation", "malformed-line"])
@pytest.mark.parametrize("odd", [False, True], ids=["ordinary", "zero-length-and-inverted"])
@pytest.mark.parametrize("opts", [["-S", "-i"], ["-S"], ["-S", "-gaps"]], ids=lambda o: " ".join(o))
def test_the_stop_is_the_class_layers(tmp_path, opts, odd, tail):
    """randomized -S inputs whose last reference region lies well before the last queries, an offending line appended behind all:
    exit status, message and output are what the reference's subset loop does on the class layer -- which stops reading at
    Done() without -inv (exit 0) and reads on to the error with it"""
    rng = np.random.default_rng(5 + len(opts) + 2 * odd)
    refs = bed_lines(rng, 400, 250_000, 400, prefix="r")
    lines = bed_lines(rng, 40_000, 400_000, 400)
    if odd:
        refs, lines = blur(rng, refs, 0.05, 0.05), blur(rng, lines, 0.01, 0.01)
    lines.append("chr1\t5\t9\tlate\t0\t+" if tail == "order-violation" else "chr3\t399999")
    write(tmp_path / "r.bed", refs); write(tmp_path / "q.bed", lines)
    for inv in ([], ["-inv"]):
        rc_c, out_c, err_c = caller(opts + inv + ["r.bed", "q.bed"], tmp_path)
        assert rc_c == (1 if inv else 0), err_c                                # the stop decides
        read = [r.split("\t") for r in out_c.splitlines()]
        assert (len(read) == len(lines) - 1) == bool(inv)                     # without -inv the loop ends before the end of the file
        want = "".join(render(lines[int(no) - 1]) for no, keep in read if keep == "1")
        for name, env in WAYS:
            rc, out, err, trace = tool(opts + inv + ["r.bed", "q.bed"], tmp_path, env)
            assert (rc, err.strip()) == (rc_c, err_c.strip()), (name, err)
            assert out == want, name
            assert (trace is None) == (name == "loop")
        # whether walking every match (as overlap does) stops the loop elsewhere than the single call: reported, not required
        rc_f, out_f, _ = caller(opts + inv + ["-full", "r.bed", "q.bed"], tmp_path)
        print("single call and full walk read the same queries:", [r[0] for r in read] == [r.split("\t")[0] for r in out_f.splitlines()], opts, inv, odd)
