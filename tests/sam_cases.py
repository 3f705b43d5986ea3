"""A plain restatement of how a block of SAM alignments becomes packed triples, and the case tables of the SAM tokenizer tests.

Not a test file.  tests/test_sam_cases_cpu.py pins `expected` to gtx_packtool --sam (the host packer, csrc/gtx_bed.cpp), to the
independent reader of tests/sam_text.py and to the oracle's CLI; tests/test_gpu_sam_seams.py then holds the device tokenizer
(text_parse_kernel<true> of csrc/gtx_text.hip) to it.  Plain loops over bytes: nothing here calls into gtx or oracle.

The rules restated (csrc/gtx_bed.cpp: ParseSamLine, and ParsePiece's SAM branch):
  * a line is a C string: it ends at its first NUL
  * it is cut at tabs; blanks in front of a token are skipped; a trailing tab adds no token, nor do blanks alone behind the last tab;
    fewer than 11 tokens are an error
  * FLAG, POS and QNAME (the label) are read by atol (text_cases.atol); the strand is '-' iff FLAG & 0x10
  * the CIGAR is a list of (digits, operation): an operation outside M I D N S H P - X is an error ('=' is one); no digits read as 0;
    digits at the end are an operation that is found in every set, and the CIGAR ends there; "*" reads as "<strlen(SEQ)>M"
  * unless SEQ is "*", strlen(SEQ) must equal the sum over M I S X: the fragment check
  * the reference length is the sum over M D X; an N closes an interval and opens the next one
  * no interval of positive length: an error; several intervals (a spliced read): not a packed triple -- the host packer of the
    plain counting path reports the line, and so it is an ERROR here
  * from there on (name = RNAME, start = POS, stop = POS + reference length - 1, strand, label) goes through the BED rules of
    tests/text_cases.py: the 32-bit coordinate limit, the order key, the per-mode validity, min(max_label, label), the int32 weight
"""
import functools
import random

import text_cases as tc
from text_cases import ERROR, NAMES, Probe, atol
from text_cases import K_LANE, K_LINES, K_PREV_MAX, K_SEG                  # noqa: F401  (the kernels' constants, the same for SAM)
from text_cases import depth, grouped, lines_of, unit_refs                 # noqa: F401  (nothing about them depends on the format)

K_LDS_SAM = 72 * 1024                      # kLdsSam of csrc/gtx_text.hip: a parse block stages up to K_LDS_SAM - 32 bytes
SPLICED = "SPLICED"

CIGAR_OPS = b"MIDNSHP-X"
REF_OPS = b"MDX"                           # ('=' is in the reference's sets, but never gets past the tokenizer)
FRAG_OPS = b"MISX"
_U64 = 1 << 64


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def cigar_ops(cigar):
    """[(length, operation byte; 0 for digits at the end)], or None for an operation the tokenizer refuses"""
    ops, p, n = [], 0, len(cigar)
    while p < n:
        d = p
        while p < n and 0x30 <= cigar[p] <= 0x39:
            p += 1
        op = cigar[p] if p < n else 0
        if op != 0 and op not in CIGAR_OPS:
            return None
        ops.append((atol(cigar[d:p]), op))
        if op == 0:
            break
        p += 1
    return ops


@functools.lru_cache(maxsize=None)
def read_alignment(line):
    """One alignment line (without its newline) as ParseSamLine reads it: ERROR, SPLICED, or (name, start, stop, strand, label)."""
    s = tc.c_string(line)
    if tc.count_tokens(s, 0x09) < 11:
        return ERROR
    cur = tc.Cursor(s, 0x09)
    qname = cur.take()
    flag = atol(cur.take()) % _U64
    rname = cur.take()
    pos = atol(cur.take())
    cur.take()                                                    # MAPQ
    cigar = cur.take()
    cur.take(), cur.take(), cur.take()                            # RNEXT, PNEXT, TLEN
    seq = cur.take()
    strand = "-" if flag & 0x10 else "+"
    if cigar == b"*":
        cigar = b"%dM" % len(seq)
    ops = cigar_ops(cigar)
    if ops is None:
        return ERROR
    if seq != b"*" and len(seq) != sum(n for n, op in ops if op == 0 or op in FRAG_OPS):
        return ERROR
    intervals, start, ref = [], pos, 0
    for n, op in ops:
        if op != 0x4e:                                            # not N
            if op == 0 or op in REF_OPS:
                ref += n
        else:
            intervals.append((start, start + ref - 1))
            start, ref = start + ref + n, 0
    if ref > 0:
        intervals.append((start, start + ref - 1))
    if not intervals:
        return ERROR
    if len(intervals) > 1:
        return SPLICED
    return tc.checked(rname, intervals[0][0], intervals[0][1], strand, atol(qname))


def read_line(line):
    """the same for the packed path: a spliced read is reported"""
    r = read_alignment(line)
    return ERROR if r == SPLICED else r


def seam_key(block):
    return tc.seam_key(block, read_line)


def expected_blocks(blocks, mode, names, strand_aware=False, sorted_by_strand=False, max_label=1, prev=None):
    """text_cases.expected_blocks over SAM lines: per block ERROR or its kept (class, start, stop, weight), and the label sums"""
    return tc.expected_blocks(blocks, mode, names, strand_aware, sorted_by_strand, max_label, prev, read_line=read_line)


def expected(blocks, mode, names, strand_aware=False, sorted_by_strand=False, max_label=1, prev=None):
    out, sums = expected_blocks(blocks, mode, names, strand_aware, sorted_by_strand, max_label, prev)
    return out, sum(s for s in sums if s is not None)


# ---------------------------------------------------------------------------------------------------------------------------
# the probes: one line each.  In a template {c} is the chromosome and {s} the POS of the filler line the probe replaces, {ps} the
# POS of the line in front of it (0 at line 0), {cn} / {cp} the known chromosome behind / in front of {c} (text_cases.Probe).
# plain: the documented plain case of GTX_TEXT_SAM in include/gtx.h -- where the restatement finds no error, the device must keep
# the block.
# ---------------------------------------------------------------------------------------------------------------------------
BASE = dict(q=b"3", f=b"0", c=b"{c}", p=b"{s}", mq=b"60", cg=b"8M", rn=b"=", pn=b"0", tl=b"0", seq=b"ACGTACGT", ql=b"IIIIIIII")
COLUMNS = ("q", "f", "c", "p", "mq", "cg", "rn", "pn", "tl", "seq", "ql")
COLUMN_NAMES = ("QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT", "TLEN", "SEQ", "QUAL")


def sam(tags=(), tail=b"", cols=11, **over):
    """the base alignment (8M at POS {s} of {c}, '+', label 3) with some columns replaced, `tags` behind QUAL and `tail` behind all"""
    assert set(over) <= set(BASE)
    f = dict(BASE, **over)
    return b"\t".join([f[k] for k in COLUMNS[:cols]] + list(tags)) + tail


def _p(group, name, template, about, plain=False, big=False):
    return Probe(name, template, about, plain, group, big)


def _cigar(name, cg, seq, about, plain=False):
    return _p("cigar", name, sam(cg=cg, seq=seq, ql=b"*" if seq == b"*" else b"I" * len(seq)), about, plain)


def _label(name, q, about, plain=False):
    return _p("label", name, sam(q=q), about, plain)


_BLANK_INSIDE = dict(q=b"3 7", f=b"1 6", c=b"{c} x", p=b"{s} 1", mq=b"6 0", cg=b"8 M", rn=b"ch r9", pn=b"1 00", tl=b"-5 0", seq=b"ACGT ACG")

PROBES = [
    # column counts
    _p("columns", "10-columns", sam(cols=10), "10 columns: no QUAL"),
    _p("columns", "11-columns", sam(), "11 columns", plain=True),
    _p("columns", "12-columns", sam(tags=[b"NM:i:0"]), "12 columns", plain=True),
    _p("columns", "13-columns", sam(tags=[b"NM:i:0", b"AS:i:8"]), "13 columns", plain=True),
    _p("columns", "trailing-tab", sam(tail=b"\t"), "a tab behind QUAL", plain=True),
    _p("columns", "trailing-tab-tags", sam(tags=[b"NM:i:0"], tail=b"\t"), "a tab behind the last tag", plain=True),
] + [
    _p("columns", "empty-" + COLUMN_NAMES[k], sam(**{COLUMNS[k]: b""}), "an empty " + COLUMN_NAMES[k]) for k in range(10)
] + [
    _p("columns", "empty-QUAL", sam(ql=b""), "an empty QUAL at the end of the line: 10 tokens"),
    _p("columns", "empty-QUAL-tags", sam(ql=b"", tags=[b"NM:i:0"]), "an empty QUAL with a tag behind it: 12 tokens"),
    _p("columns", "one-token", b"{c}", "a line of one token"),
    _p("columns", "empty-line", b"", "an empty line"),
    # bytes
] + [
    _p("bytes", "blank-inside-" + COLUMN_NAMES[k], sam(**{COLUMNS[k]: _BLANK_INSIDE[COLUMNS[k]]}), "a blank inside " + COLUMN_NAMES[k]) for k in range(10)
] + [
    _p("bytes", "blank-before-" + COLUMN_NAMES[k], sam(**{COLUMNS[k]: b" " + BASE[COLUMNS[k]]}), "a blank in front of " + COLUMN_NAMES[k]) for k in range(10)
] + [
    _p("bytes", "blank-before-QUAL", sam(ql=b" IIIIIII"), "QUAL starting with a blank"),
    _p("bytes", "blank-QUAL", sam(ql=b"  "), "a QUAL of blanks alone at the end of the line: 10 tokens"),
    _p("bytes", "crlf-11", sam(tail=b"\r"), "a carriage return behind QUAL"),
    _p("bytes", "crlf-12", sam(tags=[b"NM:i:0"], tail=b"\r"), "a carriage return behind a tag"),
    _p("bytes", "cr-QUAL", sam(ql=b"\r"), "a QUAL that is one carriage return"),
    _p("bytes", "cr-inside-tag", sam(tags=[b"NM:i\r:0", b"AS:i:8"]), "a carriage return inside a tag", plain=True),
    _p("bytes", "nul-QNAME", sam(q=b"3\x007"), "a NUL in QNAME: the C string is one token"),
    _p("bytes", "nul-RNAME", sam(c=b"ch\x00r1"), "a NUL in RNAME"),
    _p("bytes", "nul-SEQ", sam(seq=b"ACGT\x00CGT"), "a NUL in SEQ: 10 tokens"),
    _p("bytes", "nul-QUAL-first", sam(ql=b"\x00IIIIIII"), "a NUL as QUAL's first byte: the C string has 10 tokens"),
    _p("bytes", "nul-QUAL-first-tags", sam(ql=b"\x00IIIIIII", tags=[b"NM:i:0"]), "the same with a tag behind it"),
    _p("bytes", "nul-QUAL-later", sam(ql=b"II\x00IIIII"), "a NUL later in QUAL: 11 tokens", plain=True),
    _p("bytes", "nul-tag", sam(tags=[b"NM:\x00i:0"]), "a NUL in a tag", plain=True),
    _p("bytes", "high-byte-RNAME", sam(c=b"{c}\xe9"), "a byte >= 0x80 in RNAME: sorts behind every ASCII name", plain=True),
    _p("bytes", "high-byte-QUAL", sam(ql=b"II\xff\x80IIII"), "bytes >= 0x80 in QUAL", plain=True),
    # FLAG
    _p("flag", "flag-0", sam(f=b"0"), "FLAG 0: +", plain=True),
    _p("flag", "flag-16", sam(f=b"16"), "FLAG 16: -", plain=True),
    _p("flag", "flag-272", sam(f=b"272"), "FLAG 272: -", plain=True),
    _p("flag", "flag-4", sam(f=b"4"), "FLAG 4 (unmapped): +", plain=True),
    _p("flag", "flag-32", sam(f=b"32"), "FLAG 32 (the mate's strand): +", plain=True),
    _p("flag", "flag-10-digits", sam(f=b"0000000016"), "10 digits", plain=True),
    _p("flag", "flag-11-digits", sam(f=b"00000000016"), "11 digits"),
    _p("flag", "flag-above-32-bits", sam(f=b"4294967312"), "2^32 + 16: -", plain=True),
    _p("flag", "flag-plus", sam(f=b"+16"), "+16"),
    _p("flag", "flag-minus", sam(f=b"-16"), "-16: bit 4 of its two's complement is set"),
    _p("flag", "flag-letter", sam(f=b"16x"), "16x"),
    # POS (an empty FLAG and an empty POS are among the empty columns)
    _p("pos", "pos-0", sam(p=b"0"), "POS 0", plain=True),
    _p("pos", "pos-1", sam(p=b"1"), "POS 1", plain=True),
    _p("pos", "pos-0-length-1", sam(p=b"0", cg=b"1M", seq=b"A", ql=b"I"), "POS 0, one base: stop 0"),
    _p("pos", "pos-leading-zeros", sam(p=b"00{s}"), "leading zeros", plain=True),
    _p("pos", "pos-10-digits-below", sam(p=b"2147483637"), "stop 2^31 - 4: kept", plain=True, big=True),
    _p("pos", "pos-10-digits-last", sam(p=b"2147483638"), "stop 2^31 - 3: the last one kept", plain=True, big=True),
    _p("pos", "pos-10-digits-at", sam(p=b"2147483639"), "stop 2^31 - 2: the 32-bit error", big=True),
    _p("pos", "pos-at-limit", sam(p=b"2147483646", cg=b"*", seq=b"*", ql=b"*"), "start 2^31 - 2", big=True),
    _p("pos", "pos-11-digits", sam(p=b"10000000000"), "11 digits", big=True),
    _p("pos", "pos-11-digits-small", sam(p=b"00000000600"), "11 digits that read as 600"),
    _p("pos", "pos-plus", sam(p=b"+{s}"), "a + sign"),
    _p("pos", "pos-minus", sam(p=b"-{s}"), "a - sign"),
    _p("pos", "pos-letter", sam(p=b"{s}x"), "a letter behind the digits"),
    # CIGAR
    _cigar("cigar-star-seq-star", b"*", b"*", "* with SEQ *: 1M", plain=True),
    _cigar("cigar-star-seq", b"*", b"ACGTACGT", "* with a SEQ: 8M", plain=True),
    _cigar("cigar-M", b"8M", b"ACGTACGT", "M alone", plain=True),
    _cigar("cigar-X", b"8X", b"ACGTACGT", "X alone", plain=True),
    _cigar("cigar-D-seq-star", b"8D", b"*", "D alone with SEQ *", plain=True),
    _cigar("cigar-D-seq", b"8D", b"ACGTACGT", "D alone with a SEQ: the fragment is 0"),
    _cigar("cigar-I", b"5I", b"ACGTA", "I alone: no reference length"),
    _cigar("cigar-S", b"8S", b"ACGTACGT", "S alone: no reference length"),
    _cigar("cigar-H", b"8H", b"*", "H alone: no reference length"),
    _cigar("cigar-P", b"8P", b"*", "P alone: no reference length"),
    _cigar("cigar-dash", b"8-", b"*", "- alone: no reference length"),
    _cigar("cigar-mixed", b"2H3S4M1I2D1P2-3X2S", b"ACGTACGTACGTA", "all eight: reference 9, fragment 13", plain=True),
    _cigar("cigar-0M", b"0M", b"*", "0M: no reference length"),
    _cigar("cigar-0M-8M", b"0M8M", b"ACGTACGT", "0M in front of 8M", plain=True),
    _cigar("cigar-N", b"10M5N10M", b"ACGTACGTACGTACGTACGT", "a spliced read"),
    _cigar("cigar-0N", b"5M0N5M", b"ACGTACGTAC", "a splice of length 0: still two intervals"),
    _cigar("cigar-N-last", b"8M5N", b"ACGTACGT", "an N at the end: one interval"),
    _cigar("cigar-equals", b"5=5M", b"ACGTACGTAC", "=: refused"),
    _cigar("cigar-digits-last", b"5M5", b"ACGTACGTAC", "digits at the end: an operation found in every set"),
    _cigar("cigar-digits-only", b"50", b"A" * 50, "digits alone"),
    _cigar("cigar-op-only", b"M", b"*", "an operation without digits: length 0"),
    _cigar("cigar-MM", b"5MM", b"ACGTA", "5M and an M of length 0"),
    _cigar("cigar-9-digits", b"000000008M", b"ACGTACGT", "9 digits", plain=True),
    _cigar("cigar-9-digits-long", b"8M100000000D", b"ACGTACGT", "a deletion of 10^8 bases", plain=True),
    _cigar("cigar-10-digits", b"0000000008M", b"ACGTACGT", "10 digits"),
    _cigar("cigar-lower-case", b"8m", b"ACGTACGT", "a lower-case m"),
    _cigar("cigar-star-5M", b"*5M", b"ACGTA", "*5M"),
    _cigar("cigar-blank-last", b"8M ", b"ACGTACGT", "a blank behind the last operation"),
    # SEQ against the CIGAR
    _cigar("seq-equal", b"8M", b"ACGTACGT", "as long as the fragment", plain=True),
    _cigar("seq-short", b"8M", b"ACGTACG", "one short"),
    _cigar("seq-long", b"8M", b"ACGTACGTA", "one long"),
    _cigar("seq-star", b"2S6M3I", b"*", "* with a CIGAR: not checked", plain=True),
    _cigar("seq-S-I-counted", b"2S4M2I", b"ACGTACGT", "soft clip and insertion are part of the fragment", plain=True),
    _cigar("seq-S-I-left-out", b"2S4M2I", b"ACGT", "... and a SEQ without them is not"),
    _cigar("seq-H-P-D-not-counted", b"2H8M1P2D", b"ACGTACGT", "H, P and D are not", plain=True),
    _cigar("seq-H-counted", b"2H8M", b"ACGTACGTAC", "a SEQ that counts the hard clip"),
    _cigar("seq-D-counted", b"6M2D", b"ACGTACGT", "a SEQ that counts the deletion"),
    _cigar("seq-X-counted", b"5M3X", b"ACGTACGT", "X is part of the fragment and of the reference", plain=True),
    # labels (QNAME under max_label > 1)
    _label("label-7", b"7", "7", plain=True),
    _label("label-7up", b"7up", "7up", plain=True),
    _label("label--3", b"-3", "-3", plain=True),
    _label("label-+4", b"+4", "+4", plain=True),
    _label("label-x", b"x", "no digits: 0", plain=True),
    _label("label-int32-max", b"2147483647", "2147483647", plain=True),
    _label("label-int32-max+1", b"2147483648", "2147483648", plain=True),
    _label("label-int32-min", b"-2147483648", "-2147483648", plain=True),
    _label("label-int32-min-1", b"-2147483649", "-2147483649: no int32 weight"),
    _label("label-18-digits", b"999999999999999999", "18 digits", plain=True),
    _label("label-19-digits", b"9999999999999999999", "19 digits: wraps below zero"),
    _label("label-control-byte", b"\x0b7", "a vertical tab in front: atol skips it"),
    # chromosomes
    _p("chrom", "unknown-chrom", sam(c=b"chr1_x"), "an unknown chromosome that sorts between chr10 and chr2", plain=True),
    _p("chrom", "star-chrom", sam(c=b"*"), "RNAME *: sorts in front of every known one", plain=True),
    _p("chrom", "prefix-chrom", sam(c=b"chr"), "a proper prefix of every known name", plain=True),
    _p("chrom", "longer-chrom", sam(c=b"{c}0"), "the known name with a 0 behind it", plain=True),
    _p("chrom", "stop-0-unknown", sam(c=b"chr1_x", p=b"0", cg=b"1M", seq=b"A", ql=b"I"), "stop 0 on an unknown chromosome: dropped before it is validated", plain=True),
    # order
    _p("order", "equal-pos", sam(p=b"{ps}"), "the POS of the line before", plain=True),
    _p("order", "pos-lower-by-1", sam(p=b"{ps-1}"), "one below the POS of the line before"),
    _p("order", "chrom-forward", sam(c=b"{cn}"), "the next chromosome early"),
    _p("order", "chrom-backward", sam(c=b"{cp}"), "the chromosome before, again"),
    _p("order", "strand-back", sam(f=b"0"), "FLAG 0 (behind - lines, under sorted_by_strand, that is late)", plain=True),
    _p("order", "strand-forward", sam(f=b"16"), "FLAG 16 (in front of + lines, under sorted_by_strand, the NEXT line is late)", plain=True),
]
PROBE = {p.name: p for p in PROBES}
assert len(PROBE) == len(PROBES)
ORDER_PROBES = [p for p in PROBES if p.group == "order" and not p.name.startswith("strand-")]


# ---------------------------------------------------------------------------------------------------------------------------
# filler and placements
# ---------------------------------------------------------------------------------------------------------------------------
_BASES = "ACGTN"
_FLAGS = {"+": (0, 256, 1, 2048), "-": (16, 272, 17, 2064)}


@functools.lru_cache(maxsize=None)
def filler_line(f, cols=None):
    """the plain alignment of one text_cases.filler_fields entry (chromosome, col2, col3, label, strand): POS = col2, reference length
    col3 - col2 (3..13), QNAME the label; CIGAR, SEQ, FLAG and the column count (11, 12 or 13 unless `cols` says) vary with the line"""
    c, s, e, lab, strand = f
    g, n = s - 2, e - s
    kind = g % 5
    if kind == 0:
        cigar, frag = "%dM" % n, n
    elif kind == 1:
        cigar, frag = "2S%dM" % n, n + 2
    elif kind == 2:
        cigar, frag = "1M1I%dM" % (n - 1), n + 1
    elif kind == 3:
        cigar, frag = "1M1D%dX" % (n - 2), n - 1
    else:
        cigar, frag = "*", n
    seq = "*" if kind != 4 and g % 7 == 3 else "".join(_BASES[(g + k) % 5] for k in range(frag))
    qual = "*" if seq == "*" else "I" * len(seq)
    cols = 11 + g % 3 if cols is None else cols
    tok = [str(lab), str(_FLAGS[strand][g % 4]), c, str(s), "60", cigar, "=", str(s + 200), "0", seq, qual, "NM:i:0", "AS:i:%d" % frag]
    return "\t".join(tok[:cols]).encode()


def _pad(line, k):
    """the filler line k bytes longer: more text in its last column (QUAL or a tag; neither is looked at)"""
    return line + b"p" * k


def place(probe, j, n_lines, **kw):
    """text_cases.place over SAM filler lines"""
    kw.setdefault("cols", None)
    return tc.place(probe, j, n_lines, filler_line=filler_line, _pad=_pad, **kw)


def stretched(lines, total_bytes):
    return tc.stretched(lines, total_bytes, _pad=_pad)


def long_line(f, size):
    """the filler alignment of `f` in `size` bytes, most of them a soft clip: CIGAR <k>S<n>M with a SEQ and a QUAL of k + n bytes"""
    c, s, e, lab, strand = f
    n = e - s
    head = "%s\t%d\t%s\t%d\t60\t" % (lab, _FLAGS[strand][0], c, s)
    k = (size - len(head) - 64) // 2
    assert k > 0
    line = (head + "%dS%dM\t=\t0\t0\t%s\t%s\tNM:i:0" % (k, n, "A" * (k + n), "I" * (k + n))).encode()
    assert len(line) <= size
    return _pad(line, size - len(line))


# ---------------------------------------------------------------------------------------------------------------------------
# the fuzz generator
# ---------------------------------------------------------------------------------------------------------------------------
def fuzz_blocks(seed, n_blocks, probes=None):
    """n_blocks independent blocks of 1..300 lines: every even-numbered block clean, every other one with exactly one line replaced
    by a random probe at a random line.  Returns [(block, probe or None, line)]."""
    rng = random.Random(seed)
    probes = [p for p in PROBES if not p.big] if probes is None else probes
    out = []
    for b in range(n_blocks):
        n = rng.randint(1, 300)
        if b % 2 == 0:
            out.append((place(None, 0, n), None, -1))
        else:
            p, j = rng.choice(probes), rng.randrange(n)
            out.append((place(p, j, n), p, j))
    return out
