"""CPU suite: tests/gff_cases.py pinned before the GPU tests trust it.

  * hand-derived readings of single lines and first lines, each with the lines of the reference it restates
    (gtools/genomic_intervals.cpp: GenomicRegionGFF::Read :3501-3517, ProcessFileHeader :3713-3730, DetectFileFormat :3736-3759;
    CountTokens / GetNextToken core.cpp:577-625)
  * every probe, in every mode and option of gtx_packtool --gff, against the host packer on the same bytes: triples, weights, the
    line count and exit status 0 against 1
  * against an independent reading: tests/gff_text.py (a str reader written from the reference's reader) gives the same region or
    raises, and its BED6 restatement of the block, pushed through tests/text_cases.py, gives the same triples
  * the probes the oracle's CLI can express, against `gtx_oracle count` on that BED restatement over one unit-width region per base
  * the generator of the GPU fuzz test: at least half of its blocks are clean, and the host packer accepts every clean one
"""
import itertools
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import gff_cases as gc
import gff_text as gt
import text_cases as tc
from oracle import orc
from test_text_cases_cpu import REF_ORDERS, unit_ref_files      # noqa: F401  (the fixture: one unit-width region per base, four file orders)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "gtx_packtool")

OPTIONS = [c for c in itertools.product((False, True), repeat=3)]          # (-a, -s, -l 5)


def pack(mode, block, strand_aware, by_strand, max_label):
    args = [TOOL, mode, "--gff", "-t", "1", "-c", ",".join(tc.NAMES)] + (["-a"] if strand_aware else []) + (["-s"] if by_strand else [])
    args += ["-l", str(max_label)] if max_label > 1 else []
    r = subprocess.run(args, input=block, capture_output=True)
    out = r.stdout.decode().splitlines()
    rows = [tuple(int(x) for x in l.split()) for l in out if l and not l.startswith("#")]
    return r.returncode, rows, [l for l in out if l.startswith("#")], r.stderr.decode()


def check_against_packer(block, mode, strand_aware, by_strand, max_label, what):
    (want,), _ = gc.expected([block], mode, tc.NAMES, strand_aware, by_strand, max_label)
    rc, rows, meta, err = pack(mode, block, strand_aware, by_strand, max_label)
    if want == tc.ERROR:
        assert rc == 1, (what, rows[-3:], err)
        return
    assert rc == 0, (what, err)
    want = tc.grouped(want, len(tc.NAMES)) if strand_aware else want
    assert rows == [k if max_label > 1 else k[:3] for k in want], what
    assert meta == ["# lines=%d" % block.count(b"\n")], what


def _line(**kw):
    return gc.gff(**kw).replace(b"{c}", b"chr1").replace(b"{s}", b"100").replace(b"{e}", b"110")


def test_the_reader_on_hand_derived_lines():
    r = gc.read_feature
    # :3509-3510, :3516: START and END as written, no -1 and no +1; :3514: the label is column 9
    assert r(_line()) == (b"chr1", 100, 110, "+", 3)
    assert r(b"chrX\tensembl\tgene\t1\t1\t.\t-\t0\t42\tc") == (b"chrX", 1, 1, "-", 42)
    # :3504-3505: 8, 9 or 10 tokens; :3514: "_" with 8 -- a label value of 0
    assert r(_line(cols=7)) == tc.ERROR and r(_line(cols=10, tail=b"\tx")) == tc.ERROR
    assert r(_line(cols=8)) == (b"chr1", 100, 110, "+", 0) and r(_line(cols=10)) == (b"chr1", 100, 110, "+", 3)
    # core.cpp:586-589: a trailing tab adds no token, nor do blanks alone behind the last tab; an empty token inside counts
    assert r(_line(cols=10, tail=b"\t")) != tc.ERROR and r(_line(cols=8, tail=b"\t"))[4] == 0 and r(_line(cols=7, tail=b"\t")) == tc.ERROR
    assert r(_line(cols=10, cm=b"  "))[4] == 3 and r(_line(cols=10, lab=b""))[4] == 0 and r(_line(cols=10, s=b""))[1] == 0
    # core.cpp:616: blanks in front of a token are skipped
    assert r(_line(c=b"  chr1", s=b" 100", st=b" -")) == (b"chr1", 100, 110, "-", 3)
    # :3512: the first byte of column 7, kept raw ('.' is not BED's '+'); an empty column is the NUL of an empty C string
    assert [r(_line(st=s))[3] for s in (b"+", b"-", b".", b"?", b"1", b"+-", b"-1", b"")] == ["+", "-", ".", "?", "1", "+", "-", "\0"]
    # atol (:3509-3510, :1081-1085): a sign, digits, the rest ignored; a GTF attribute string reads as 0
    assert r(_line(s=b"-5"))[1] == -5 and r(_line(s=b"+7x"))[1] == 7 and r(_line(e=b"00000000640"))[2] == 640
    assert r(_line(lab=b'gene_id "G1"; level 2;'))[4] == 0 and r(_line(lab=b"7up"))[4] == 7 and r(_line(lab=b"-3"))[4] == -3 and r(_line(lab=b"_"))[4] == 0
    assert r(_line(lab=b"999999999999999999"))[4] == 999999999999999999 and r(_line(lab=b"9999999999999999999"))[4] < 0
    # a C string ends at a NUL
    assert r(_line(c=b"ch\x00r1")) == tc.ERROR and r(_line(lab=b"3\x004"))[4] == 3 and r(_line(lab=b"\x003"))[4] == 0
    # the packed path's 32-bit limit: 2^31 - 3 is the last coordinate kept
    assert r(_line(s=b"2147483644", e=b"2147483645"))[2] == 2147483645 and r(_line(s=b"2147483644", e=b"2147483646")) == tc.ERROR
    assert r(b"#a comment") == tc.ERROR and r(b"##gff-version 3") == tc.ERROR and r(b"") == tc.ERROR


def test_the_strand_rule_and_the_modes():
    e = lambda text, mode, **kw: gc.expected([text], mode, tc.NAMES, **kw)[0][0]
    dot = _line(st=b".") + b"\n"
    # with the strand ignored any byte goes; a strand-aware run reports the line
    assert e(dot, "ou") == [(0, 100, 110, 1)] and e(dot, "os") == [(0, 100, 110, 1)]
    assert e(dot, "ou", strand_aware=True) == tc.ERROR and e(dot, "ss", strand_aware=True) == tc.ERROR
    assert e(_line(st=b"?") + b"\n", "su") == [(0, 100, 110, 1)] and e(_line(st=b"") + b"\n", "ou", strand_aware=True) == tc.ERROR
    assert e(_line(st=b"-") + b"\n", "ou", strand_aware=True) == [(3, 100, 110, 1)]
    # ... also for a feature of a chromosome no reference region has: the line is read before it is dropped
    assert e(_line(c=b"chrQ", st=b".") + b"\n", "ou") == [] and e(_line(c=b"chrQ", st=b".") + b"\n", "ou", strand_aware=True) == tc.ERROR
    # the unsorted overlap rules report START > END and END <= 0, the unsorted scanner drops them, the sorted rules keep them
    odd = _line(s=b"112") + b"\n"
    assert e(odd, "ou") == tc.ERROR and e(odd, "su") == [] and e(odd, "os") == [(0, 112, 110, 1)]
    # the order key is (seqname, [strand,] START); a dropped line's key counts
    two = _line(c=b"chr1_x") + b"\n" + _line(c=b"chr10", s=b"5") + b"\n"
    assert e(_line() + b"\n" + two, "os") == tc.ERROR and e(_line() + b"\n" + two, "ou") == [(0, 100, 110, 1), (1, 5, 110, 1)]
    assert e(_line(st=b"-") + b"\n" + _line() + b"\n", "os", strand_aware=True, sorted_by_strand=True) == tc.ERROR
    assert e(_line(st=b"-") + b"\n" + _line() + b"\n", "os", strand_aware=True) == [(3, 100, 110, 1), (0, 100, 110, 1)]
    # min(max_label, atol(column 9)); the sum takes the lines of unknown chromosomes too
    assert gc.expected([_line(lab=b"7") + b"\n" + _line(lab=b"2", c=b"chrQ") + b"\n" + _line(cols=8) + b"\n"], "ou", tc.NAMES, max_label=5) == (
        [[(0, 100, 110, 5), (0, 100, 110, 0)]], 7)


@pytest.mark.parametrize("name,line,fmt,why", gc.DETECT, ids=[d[0] for d in gc.DETECT])
def test_detection_on_hand_derived_first_lines(name, line, fmt, why):
    assert gc.detect(line) == fmt, why
    if fmt in ("GFF", "BED") and not line.startswith(b"#"):
        assert gt.looks_like_gff(line.decode()) == (fmt == "GFF"), why


@pytest.mark.parametrize("mode", tc.MODES)
def test_every_probe_in_every_mode_is_what_the_host_packer_makes_of_it(mode):
    jobs = []
    for strand_aware, by_strand, weighted in OPTIONS:
        for p in gc.PROBES:
            for block in (p.line() + b"\n", gc.place(p, "last", 300)):
                jobs.append((block, mode, strand_aware, by_strand, 5 if weighted else 1, (p, mode, strand_aware, by_strand, weighted, len(block))))
    with ThreadPoolExecutor(8) as pool:                            # (a process per case: the waiting overlaps)
        list(pool.map(lambda j: check_against_packer(*j), jobs))


LATE_MAKER = tc.Probe("late-maker", gc.gff(c=b"{c}_x"), "an unknown chromosome that sorts behind {c}")


@pytest.mark.parametrize("mode", ("os", "ou"))
def test_probes_inside_a_block_are_what_the_host_packer_makes_of_them(mode):
    """the probe with filler behind it too (the order probes make the NEXT line late), at the line positions the GPU test uses"""
    jobs = [(gc.place(p, j, 300), mode, aware, mode == "os" and aware, 5, (p, j, aware)) for p in gc.PROBES for j in (0, 1, 128, 257) for aware in (False, True)]
    for j in (1, 128):                                              # the late line behind an unknown chromosome, as the GPU test builds it
        for p in gc.ORDER_PROBES + [None]:
            jobs.append((gc.place(p, j, 300, extra={j - 1: LATE_MAKER}), mode, True, mode == "os", 5, (p, j, "late-maker")))
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda j: check_against_packer(*j), jobs))


def test_error_messages_of_the_host_packer():
    """what follows "Error: Line N: ": the reference's words for the token count, this build's for the strand"""
    rc, rows, meta, err = pack("ou", gc.place(gc.PROBE["11-columns"], 7, 20), False, False, 1)
    assert (rc, err) == (1, "\nError: Line 8: wrong number of tokens for GFF format!\n")
    rc, rows, meta, err = pack("os", gc.place(gc.PROBE["strand-dot"], 3, 20), True, False, 1)
    assert (rc, err) == (1, "\nError: Line 4: GFF strand '.' is neither '+' nor '-': such a feature is counted only when the strand is ignored (-i)!\n")
    rc, rows, meta, err = pack("su", gc.place(gc.PROBE["empty-strand"], 0, 20), True, False, 1)
    assert (rc, err) == (1, "\nError: Line 1: GFF strand 0x00 is neither '+' nor '-': such a feature is counted only when the strand is ignored (-i)!\n")


# ---- the independent reading ------------------------------------------------------------------------------------------------
GFF_TEXT_SKIPS = {p.name: "a str does not end at a NUL" for p in gc.PROBES if b"\x00" in p.template}


def test_every_probe_reads_as_gff_text_reads_it():
    compared = 0
    for p in gc.PROBES:
        if p.name in GFF_TEXT_SKIPS:
            continue
        line = p.line()
        mine = gc.read_feature(line)
        try:
            chrom, strand, label, start, stop = gt.read_gff(line.decode("latin-1"))
        except ValueError:
            assert mine == tc.ERROR, p
            continue
        if start >= tc.INT_MAX - 1 or stop >= tc.INT_MAX - 1:
            assert mine == tc.ERROR and p.big, p
            continue
        assert mine != tc.ERROR and mine[:4] == (chrom.encode("latin-1"), start, stop, strand or "\0"), p
        assert mine[4] == tc.atol(label.encode("latin-1")), p
        compared += 1
    assert compared > len(gc.PROBES) // 2


def to_bed_block(block, aware):
    """the block's BED6 restatement by tests/gff_text.py (bytes as Latin-1), or None where a line has none: the reader raises, or the
    strand byte is one BED spells otherwise ('.' is BED's '+': the same region only where the strand is ignored)"""
    out = []
    for k, line in enumerate(tc.lines_of(block)):
        try:
            strand = gt.read_gff(line.decode("latin-1"))[1]
            if len(strand) != 1 or strand not in ("+-" if aware else "+-."):
                return None
            out.append(gt.to_bed(line.decode("latin-1"), k, numeric_label=True).encode("latin-1"))
        except ValueError:
            return None
    return b"\n".join(out) + b"\n"


@pytest.mark.parametrize("mode", tc.MODES)
def test_the_bed_restatement_of_every_probe_gives_the_same_triples(mode):
    compared = 0
    for p in gc.PROBES:
        if p.name in GFF_TEXT_SKIPS:
            continue
        for j in (150, "last"):
            block = gc.place(p, j, 300)
            for strand_aware, by_strand, weighted in OPTIONS:
                bed = to_bed_block(block, strand_aware or by_strand)
                if bed is None:
                    continue
                want = gc.expected([block], mode, tc.NAMES, strand_aware, by_strand, 5 if weighted else 1)
                assert tc.expected([bed], mode, tc.NAMES, strand_aware, by_strand, 5 if weighted else 1) == want, (p, j, strand_aware, by_strand, weighted)
                compared += 1
    assert compared > len(gc.PROBES) * 8


# ---- the oracle's CLI -------------------------------------------------------------------------------------------------------
ORACLE_SKIPS_WEIGHTED = {"label-int32-min-1", "label-19-digits"}      # the oracle adds what no int32 weight can hold; the packed path reports the line


@pytest.mark.parametrize("opts", (["-i"], [], ["-S", "-i"], ["-S"], ["-S", "-s"]), ids=" ".join)
def test_restated_depth_is_what_the_oracle_prints(unit_ref_files, opts):
    d, orders = unit_ref_files
    aware, mode = "-i" not in opts, "os" if "-S" in opts else "ou"
    n_classes = len(tc.NAMES) * (2 if aware else 1)
    ref_file = "refs_by_strand.bed" if "-s" in opts else "refs_by_pos.bed" if opts == ["-S"] else "refs_aware.bed" if aware else "refs.bed"
    compared = errors = 0
    for weighted in (False, True):
        for p in gc.PROBES:
            if p.big or p.name in GFF_TEXT_SKIPS or (weighted and p.name in ORACLE_SKIPS_WEIGHTED):
                continue
            block = gc.place(p, 150, 300)
            bed = to_bed_block(block, aware)
            if bed is None:                                       # no BED line says it (the other tests hold the restated ERROR)
                continue
            (want,), _ = gc.expected([block], mode, tc.NAMES, aware, "-s" in opts, 5 if weighted else 1)
            (d / "reads_gff.bed").write_bytes(bed)
            r = subprocess.run([orc.CLI, "count"] + opts + (["--max-label-value", "5"] if weighted else []) + [ref_file, "reads_gff.bed"], capture_output=True, cwd=d)
            if want == tc.ERROR:
                assert r.returncode == 1, (p, weighted)
                errors += 1
                continue
            assert r.returncode == 0, (p, weighted, r.stderr.decode())
            got = [int(l.split("\t")[1]) for l in r.stdout.decode().splitlines()]
            depth = tc.depth([want], n_classes)
            assert got == [depth[i] for i in orders[ref_file]], (p, weighted)
            compared += 1
    assert compared > len(gc.PROBES) // 2 and (errors > 0 or mode == "ou")


# ---- placements and the generator --------------------------------------------------------------------------------------------
def test_filler_and_placements():
    fields = tc.filler_fields(300)
    lines = [gc.filler_line(f) for f in fields]
    assert {l.count(b"\t") + 1 for l in lines} == {8, 9, 10}
    got = [gc.read_feature(l) for l in lines]
    assert all(g != tc.ERROR and 1 <= g[1] <= g[2] <= tc.L for g in got)
    assert {g[3] for g in got} == {"+", "-"} and [g[1] for g in got] == sorted(g[1] for g in got)
    assert [(g[0].decode(), g[1], g[2], g[3]) for g in got] == [(f[0], f[1], f[2], f[4]) for f in fields]
    assert [g[4] for g, l, f in zip(got, lines, fields)] == [f[3] if l.count(b"\t") >= 8 else 0 for l, f in zip(lines, fields)]
    assert any(b"gene_id" in l for l in lines)
    for mode, aware, by_strand in (("os", True, True), ("os", False, False), ("ou", True, False)):
        (want,), _ = gc.expected([gc.place(None, 0, 300)], mode, tc.NAMES, aware, by_strand, 5)
        assert want != tc.ERROR and len(want) == 300
    p = gc.PROBE["crlf-9"]
    for at in tc.NEWLINE_OFFSETS[2:]:
        for j in (1, 2, 9):
            b = gc.place(p, j, 200, newline_at=at)
            assert b[at:at + 1] == b"\n" and b[:at].count(b"\n") == j and b[at - 1:at] == b"\r"
    for m, rs in ((16, tc.LEN_MOD_16), (1024, tc.LEN_MOD_1024)):
        for r in rs:
            for j in (0, 5, "last"):
                b = gc.place(p, j, 130, total_bytes_mod=(m, r))
                assert len(b) % m == r and b.count(b"\n") == 130
    for size in (4000, 4096, 5000):
        f = fields[40]
        l = gc.long_line(f, size)
        assert len(l) == size and gc.read_feature(l)[:4] == gc.read_feature(gc.filler_line(f))[:4]
    lines = gc.stretched([gc.filler_line(f) for f in tc.filler_fields(128)], gc.K_LDS_GFF - 32)
    assert sum(len(l) + 1 for l in lines) == gc.K_LDS_GFF - 32


FUZZ = {"ou": (31, 120), "os": (32, 120), "os-by-strand": (33, 120), "ou-weighted": (34, 120), "os-strands-weighted": (35, 120)}      # (seed, blocks): the GPU test's
FUZZ_RULES = {"ou": ("ou", False, False, 1), "os": ("os", False, False, 1), "os-by-strand": ("os", True, True, 1), "ou-weighted": ("ou", False, False, 5),
              "os-strands-weighted": ("os", True, False, 5)}


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_generator_blocks_are_clean_at_least_half_the_time_and_the_host_packer_takes_them(name):
    seed, n = FUZZ[name]
    mode, aware, by_strand, max_label = FUZZ_RULES[name]
    blocks = gc.fuzz_blocks(seed, n)
    assert blocks == gc.fuzz_blocks(seed, n)
    clean = [b for b, p, _ in blocks if p is None]
    assert 2 * len(clean) >= len(blocks) and len(blocks) == n
    assert all(1 <= b.count(b"\n") <= 300 for b, _, _ in blocks)
    jobs = []
    for b in clean:
        (want,), _ = gc.expected([b], mode, tc.NAMES, aware, by_strand, max_label)
        assert want != tc.ERROR and len(want) == b.count(b"\n")
        jobs.append((b, mode, aware, by_strand, max_label, name))
    # ... and the blocks with a probe are what the host packer makes of them, too
    jobs += [(b, mode, aware, by_strand, max_label, (name, p, j)) for b, p, j in blocks[1::2][:40]]
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda j: check_against_packer(*j), jobs))
