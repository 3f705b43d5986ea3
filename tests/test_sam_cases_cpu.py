"""CPU suite: tests/sam_cases.py pinned before the GPU tests trust it.

  * every probe, in every mode and option of gtx_packtool --sam, against the host packer on the same bytes: triples, weights, the
    line count and exit status 0 against 1
  * against an independent reading: tests/sam_text.py (a str reader written from the reference's GenomicRegionSAM::Read) gives the
    same region or raises, and its BED6 restatement of the block, pushed through tests/text_cases.py, gives the same triples
  * the probes the oracle's CLI can express, against `gtx_oracle count` on that BED restatement over one unit-width region per base
  * the generator of the GPU fuzz test: at least half of its blocks are clean, and the host packer accepts every clean one
"""
import itertools
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import sam_cases as sc
import sam_text as st
import text_cases as tc
from oracle import orc
from test_text_cases_cpu import REF_ORDERS, unit_ref_files      # noqa: F401  (the fixture: one unit-width region per base, four file orders)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "gtx_packtool")

OPTIONS = [c for c in itertools.product((False, True), repeat=3)]          # (-a, -s, -l 5)


def pack(mode, block, strand_aware, by_strand, max_label):
    args = [TOOL, mode, "--sam", "-t", "1", "-c", ",".join(tc.NAMES)] + (["-a"] if strand_aware else []) + (["-s"] if by_strand else [])
    args += ["-l", str(max_label)] if max_label > 1 else []
    r = subprocess.run(args, input=block, capture_output=True)
    out = r.stdout.decode().splitlines()
    rows = [tuple(int(x) for x in l.split()) for l in out if l and not l.startswith("#")]
    return r.returncode, rows, [l for l in out if l.startswith("#")], r.stderr.decode()


def check_against_packer(block, mode, strand_aware, by_strand, max_label, what):
    (want,), _ = sc.expected([block], mode, tc.NAMES, strand_aware, by_strand, max_label)
    rc, rows, meta, err = pack(mode, block, strand_aware, by_strand, max_label)
    if want == tc.ERROR:
        assert rc == 1, (what, rows[-3:], err)
        return
    assert rc == 0, (what, err)
    want = tc.grouped(want, len(tc.NAMES)) if strand_aware else want
    assert rows == [k if max_label > 1 else k[:3] for k in want], what
    assert meta == ["# lines=%d" % block.count(b"\n")], what


def test_the_reader_on_the_documented_outcomes():
    r = sc.read_alignment
    line = lambda **kw: sc.sam(**kw).replace(b"{c}", b"chr1").replace(b"{s}", b"100")
    assert r(line()) == (b"chr1", 100, 107, "+", 3)
    assert r(line(f=b"16")) == (b"chr1", 100, 107, "-", 3) and r(line(f=b"32"))[3] == "+" and r(line(f=b"-16"))[3] == "-"
    assert r(line(cg=b"*")) == (b"chr1", 100, 107, "+", 3) and r(line(cg=b"*", seq=b"*"))[2] == 100
    assert r(line(cg=b"2H3S4M1I2D1P2-3X2S", seq=b"ACGTACGTACGTA"))[1:3] == (100, 108)
    assert r(line(cg=b"10M5N10M", seq=b"A" * 20)) == sc.SPLICED and r(line(cg=b"5M0N5M", seq=b"A" * 10)) == sc.SPLICED
    assert r(line(cg=b"8M5N"))[1:3] == (100, 107)
    assert r(line(cg=b"5M5", seq=b"A" * 10))[2] == 109 and r(line(cg=b"50", seq=b"A" * 50))[2] == 149 and r(line(cg=b"5MM", seq=b"AAAAA"))[2] == 104
    for cg, seq in ((b"5=5M", b"A" * 10), (b"8m", b"A" * 8), (b"*5M", b"A" * 5), (b"0M", b"*"), (b"5I", b"AAAAA"), (b"M", b"*"), (b"8M", b"A" * 7),
                    (b"8M", b"A" * 9), (b"8D", b"A" * 8), (b"2H8M", b"A" * 10)):
        assert r(line(cg=cg, seq=seq)) == tc.ERROR, cg
    assert r(line(ql=b"\x00III")) == tc.ERROR and r(line(ql=b"I\x00II")) != tc.ERROR and r(line(ql=b"")) == tc.ERROR
    assert r(line(ql=b"", tags=[b"NM:i:0"])) != tc.ERROR
    assert r(line(p=b"2147483638"))[2] == 2147483645 and r(line(p=b"2147483639")) == tc.ERROR
    e = lambda text, mode, **kw: sc.expected([text], mode, tc.NAMES, **kw)[0][0]
    two = line(c=b"chr1_x") + b"\n" + line(c=b"chr10", p=b"5") + b"\n"
    assert e(line() + b"\n" + two, "os") == tc.ERROR                                           # the dropped line's key counts
    assert e(line() + b"\n" + two, "ou") == [(0, 100, 107, 1), (1, 5, 12, 1)]
    assert e(line(f=b"16") + b"\n" + line() + b"\n", "os", strand_aware=True, sorted_by_strand=True) == tc.ERROR
    assert e(line(f=b"16") + b"\n" + line() + b"\n", "os", strand_aware=True) == [(3, 100, 107, 1), (0, 100, 107, 1)]
    assert sc.expected([line(q=b"7") + b"\n" + line(q=b"2", c=b"chrQ") + b"\n"], "ou", tc.NAMES, max_label=5) == ([[(0, 100, 107, 5)]], 7)


@pytest.mark.parametrize("mode", tc.MODES)
def test_every_probe_in_every_mode_is_what_the_host_packer_makes_of_it(mode):
    jobs = []
    for strand_aware, by_strand, weighted in OPTIONS:
        for p in sc.PROBES:
            for block in (p.line() + b"\n", sc.place(p, "last", 300)):
                jobs.append((block, mode, strand_aware, by_strand, 5 if weighted else 1, (p, mode, strand_aware, by_strand, weighted, len(block))))
    with ThreadPoolExecutor(8) as pool:                            # (a process per case: the waiting overlaps)
        list(pool.map(lambda j: check_against_packer(*j), jobs))


@pytest.mark.parametrize("mode", ("os", "ou"))
def test_probes_inside_a_block_are_what_the_host_packer_makes_of_them(mode):
    """the probe with filler behind it too (the order probes make the NEXT line late), at the line positions the GPU test uses"""
    jobs = [(sc.place(p, j, 300), mode, True, mode == "os", 5, (p, j)) for p in sc.PROBES for j in (0, 1, 128, 257)]
    for j in (1, 128):                                              # the late line behind an unknown chromosome, as the GPU test builds it
        for p in sc.ORDER_PROBES + [None]:
            jobs.append((sc.place(p, j, 300, extra={j - 1: LATE_MAKER}), mode, True, mode == "os", 5, (p, j, "late-maker")))
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda j: check_against_packer(*j), jobs))


LATE_MAKER = tc.Probe("late-maker", sc.sam(c=b"{c}_x"), "an unknown chromosome that sorts behind {c}")


# ---- the independent reading ------------------------------------------------------------------------------------------------
SAM_TEXT_SKIPS = {                            # lines tests/sam_text.py (a reader of str, not of C strings) cannot express
    "nul-QNAME": "a str does not end at a NUL: the reader sees 11 columns where the C string has one",
    "nul-RNAME": "the same: the C string has three tokens",
    "nul-SEQ": "the same: the C string has 10 tokens",
    "nul-QUAL-first": "the same: the C string has 10 tokens",
    "nul-QUAL-first-tags": "the same",
}


def to_bed_block(block):
    """the block's BED6 / BED12 restatement by tests/sam_text.py (bytes as Latin-1: one code point per byte, in byte order), or None
    where a line has none (the reader raises)"""
    out = []
    for line in tc.lines_of(block):
        try:
            out.append(st.to_bed(line.decode("latin-1")).encode("latin-1"))
        except ValueError:
            return None
    return b"\n".join(out) + b"\n"


def test_every_probe_reads_as_sam_text_reads_it():
    compared = 0
    for p in sc.PROBES:
        if p.name in SAM_TEXT_SKIPS:
            continue
        line = p.line()
        mine = sc.read_alignment(line)
        try:
            chrom, strand, label, iv = st.read_sam(line.decode("latin-1"))
        except ValueError:
            assert mine == tc.ERROR, p
            continue
        if len(iv) > 1:
            assert mine == sc.SPLICED, p
            continue
        out_of_range = any(x >= tc.INT_MAX - 1 for x in iv[0])
        if out_of_range:
            assert mine == tc.ERROR and p.big, p
            continue
        assert mine != tc.ERROR and mine[:4] == (chrom.encode("latin-1"), iv[0][0], iv[0][1], strand), p
        assert mine[4] == tc.atol(label.encode("latin-1")), p
        compared += 1
    assert compared > len(sc.PROBES) // 2


@pytest.mark.parametrize("mode", tc.MODES)
def test_the_bed_restatement_of_every_probe_gives_the_same_triples(mode):
    for p in sc.PROBES:
        if p.name in SAM_TEXT_SKIPS:
            continue
        for j in (150, "last"):
            block = sc.place(p, j, 300)
            bed = to_bed_block(block)
            for strand_aware, by_strand, weighted in OPTIONS:
                want = sc.expected([block], mode, tc.NAMES, strand_aware, by_strand, 5 if weighted else 1)
                if bed is None:
                    assert want[0][0] == tc.ERROR, p
                else:
                    assert tc.expected([bed], mode, tc.NAMES, strand_aware, by_strand, 5 if weighted else 1) == want, (p, j, strand_aware, by_strand, weighted)


# ---- the oracle's CLI -------------------------------------------------------------------------------------------------------
ORACLE_SKIPS = {
    "cigar-N": "the oracle counts the BED12 region of a spliced read; the packed path reports it as outside its scope",
    "cigar-0N": "the same",
}
ORACLE_SKIPS.update(SAM_TEXT_SKIPS)
ORACLE_SKIPS_WEIGHTED = {"label-int32-min-1", "label-19-digits"}      # the oracle adds what no int32 weight can hold; the packed path reports the line


@pytest.mark.parametrize("opts", (["-i"], [], ["-S", "-i"], ["-S"], ["-S", "-s"]), ids=" ".join)
def test_restated_depth_is_what_the_oracle_prints(unit_ref_files, opts):
    d, orders = unit_ref_files
    aware, mode = "-i" not in opts, "os" if "-S" in opts else "ou"
    n_classes = len(tc.NAMES) * (2 if aware else 1)
    ref_file = "refs_by_strand.bed" if "-s" in opts else "refs_by_pos.bed" if opts == ["-S"] else "refs_aware.bed" if aware else "refs.bed"
    compared = errors = 0
    for weighted in (False, True):
        for p in sc.PROBES:
            if p.big or p.name in ORACLE_SKIPS or (weighted and p.name in ORACLE_SKIPS_WEIGHTED):
                continue
            block = sc.place(p, 150, 300)
            bed = to_bed_block(block)
            if bed is None:                                       # no BED line says it (the other tests hold the restated ERROR)
                continue
            (want,), _ = sc.expected([block], mode, tc.NAMES, aware, "-s" in opts, 5 if weighted else 1)
            (d / "reads_sam.bed").write_bytes(bed)
            r = subprocess.run([orc.CLI, "count"] + opts + (["--max-label-value", "5"] if weighted else []) + [ref_file, "reads_sam.bed"], capture_output=True, cwd=d)
            if want == tc.ERROR:
                assert r.returncode == 1, (p, weighted)
                errors += 1
                continue
            assert r.returncode == 0, (p, weighted, r.stderr.decode())
            got = [int(l.split("\t")[1]) for l in r.stdout.decode().splitlines()]
            depth = tc.depth([want], n_classes)
            assert got == [depth[i] for i in orders[ref_file]], (p, weighted)
            compared += 1
    assert compared > len(sc.PROBES) // 2 and (errors > 0 or mode == "ou")


# ---- placements and the generator --------------------------------------------------------------------------------------------
def test_filler_and_placements():
    fields = tc.filler_fields(300)
    lines = [sc.filler_line(f) for f in fields]
    assert {l.count(b"\t") + 1 for l in lines} == {11, 12, 13}
    got = [sc.read_alignment(l) for l in lines]
    assert all(g not in (tc.ERROR, sc.SPLICED) and 1 <= g[1] <= g[2] <= tc.L for g in got)
    assert {g[3] for g in got} == {"+", "-"} and [g[1] for g in got] == sorted(g[1] for g in got)
    assert [(g[0].decode(), g[1], g[2] - g[1] + 1, g[4], g[3]) for g in got] == [(f[0], f[1], f[2] - f[1], f[3], f[4]) for f in fields]
    for mode, aware, by_strand in (("os", True, True), ("os", False, False), ("ou", True, False)):
        (want,), _ = sc.expected([sc.place(None, 0, 300)], mode, tc.NAMES, aware, by_strand, 5)
        assert want != tc.ERROR and len(want) == 300
    p = sc.PROBE["crlf-12"]
    for at in tc.NEWLINE_OFFSETS[2:]:
        for j in (1, 2, 9):
            b = sc.place(p, j, 200, newline_at=at)
            assert b[at:at + 1] == b"\n" and b[:at].count(b"\n") == j and b[at - 1:at] == b"\r"
    for m, rs in ((16, tc.LEN_MOD_16), (1024, tc.LEN_MOD_1024)):
        for r in rs:
            for j in (0, 5, "last"):
                b = sc.place(p, j, 130, total_bytes_mod=(m, r))
                assert len(b) % m == r and b.count(b"\n") == 130
    for size in (4000, 4096, 5000):
        f = fields[40]
        l = sc.long_line(f, size)
        assert len(l) == size and sc.read_alignment(l)[:4] == sc.read_alignment(sc.filler_line(f))[:4]
    lines = sc.stretched([sc.filler_line(f) for f in tc.filler_fields(128)], sc.K_LDS_SAM - 32)
    assert sum(len(l) + 1 for l in lines) == sc.K_LDS_SAM - 32


FUZZ = {"ou": (21, 120), "os": (22, 120), "os-by-strand": (23, 120), "ou-weighted": (24, 120), "os-strands-weighted": (25, 120)}      # (seed, blocks): the GPU test's
FUZZ_RULES = {"ou": ("ou", False, False, 1), "os": ("os", False, False, 1), "os-by-strand": ("os", True, True, 1), "ou-weighted": ("ou", False, False, 5),
              "os-strands-weighted": ("os", True, False, 5)}


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_generator_blocks_are_clean_at_least_half_the_time_and_the_host_packer_takes_them(name):
    seed, n = FUZZ[name]
    mode, aware, by_strand, max_label = FUZZ_RULES[name]
    blocks = sc.fuzz_blocks(seed, n)
    assert blocks == sc.fuzz_blocks(seed, n)
    clean = [b for b, p, _ in blocks if p is None]
    assert 2 * len(clean) >= len(blocks) and len(blocks) == n
    assert all(1 <= b.count(b"\n") <= 300 for b, _, _ in blocks)
    jobs = []
    for b in clean:
        (want,), _ = sc.expected([b], mode, tc.NAMES, aware, by_strand, max_label)
        assert want != tc.ERROR and len(want) == b.count(b"\n")
        jobs.append((b, mode, aware, by_strand, max_label, name))
    # ... and the blocks with a probe are what the host packer makes of them, too
    jobs += [(b, mode, aware, by_strand, max_label, (name, p, j)) for b, p, j in blocks[1::2][:40]]
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda j: check_against_packer(*j), jobs))
