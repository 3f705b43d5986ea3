"""A plain restatement of how a block of GFF / GTF features becomes packed triples, of the format detection, and the case tables of the
GFF tokenizer tests.

Not a test file.  tests/test_gff_cases_cpu.py pins `expected` to gtx_packtool --gff (the host packer, csrc/gtx_bed.cpp), to the
independent reader of tests/gff_text.py and to hand-derived values; tests/test_gpu_gff_seams.py then holds the device tokenizer
(text_parse_kernel<kFmtGff>, parse_gff_line of csrc/gtx_text.hip) to it.  Plain loops over bytes: nothing here calls into gtx or oracle.

The rules restated (csrc/gtx_bed.cpp: ParseGffLine, and ParsePiece's GFF branch; the reference: GenomicRegionGFF::Read,
gtools/genomic_intervals.cpp:3501-3517, CountTokens / GetNextToken core.cpp:577-625):
  * a line is a C string: it ends at its first NUL
  * it is cut at tabs; blanks in front of a token are skipped; a trailing tab adds no token, nor do blanks alone behind the last tab;
    a token count outside 8..10 is an error ("wrong number of tokens for GFF format!")
  * START = atol(column 4), END = atol(column 5), as written: 1-based, inclusive -- no -1, no +1
  * the strand is the first byte of column 7 as it stands (NUL for an empty token): '.' is not folded into '+'
  * the label is column 9 (its atol value under max_label > 1: a GTF attribute string reads as 0), "_" -- value 0 -- with 8 tokens
  * this build's own rule: in a strand-aware run a strand byte other than '+' or '-' is an error at its line; with the strand
    ignored every byte goes
  * from there on (name, start, stop, strand, label) goes through the BED rules of tests/text_cases.py: the 32-bit coordinate
    limit, the order key, the per-mode validity, min(max_label, label), the int32 weight
"""
import functools
import random

import text_cases as tc
from text_cases import ERROR, NAMES, Probe, atol
from text_cases import K_LANE, K_LINES, K_PREV_MAX, K_SEG                  # noqa: F401  (the kernels' constants, the same for GFF)
from text_cases import depth, grouped, lines_of, unit_refs                 # noqa: F401  (nothing about them depends on the format)

K_LDS_GFF = 72 * 1024                      # kLdsSam of csrc/gtx_text.hip, which GFF shares: a parse block stages up to K_LDS_GFF - 32 bytes


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def read_feature(line):
    """One feature line (without its newline) as ParseGffLine reads it: ERROR, or (name, start, stop, strand, label), the strand a
    one-character string holding the byte as it stands ("\\0" for an empty column 7)."""
    s = tc.c_string(line)
    n = tc.count_tokens(s, 0x09)
    if n < 8 or n > 10:
        return ERROR
    cur = tc.Cursor(s, 0x09)
    name = cur.take()
    cur.take(), cur.take()                                        # source, feature
    start = atol(cur.take())
    stop = atol(cur.take())
    cur.take()                                                    # score
    strand = cur.take()[:1].decode("latin-1") or "\0"
    cur.take()                                                    # frame
    label = atol(cur.take()) if n > 8 else 0
    return tc.checked(name, start, stop, strand, label)


def read_line(line):
    """the reader of a run that ignores the strand"""
    return read_feature(line)


def read_line_aware(line):
    """the reader of a strand-aware run: a third strand is an error"""
    r = read_feature(line)
    return ERROR if r != ERROR and r[3] not in "+-" else r


def seam_key(block):
    return tc.seam_key(block, read_line)


def expected_blocks(blocks, mode, names, strand_aware=False, sorted_by_strand=False, max_label=1, prev=None):
    """text_cases.expected_blocks over GFF lines: per block ERROR or its kept (class, start, stop, weight), and the label sums"""
    return tc.expected_blocks(blocks, mode, names, strand_aware, sorted_by_strand, max_label, prev,
                              read_line=read_line_aware if strand_aware else read_line)


def expected(blocks, mode, names, strand_aware=False, sorted_by_strand=False, max_label=1, prev=None):
    out, sums = expected_blocks(blocks, mode, names, strand_aware, sorted_by_strand, max_label, prev)
    return out, sum(s for s in sums if s is not None)


def detect(first_line):
    """the format of a file by its first line (ProcessFileHeader :3713-3730, DetectFileFormat :3736-3759), as far as this build goes:
    "GFF", "SAM", "BED" or None (unsupported).  first_line: bytes without the newline."""
    s = tc.c_string(first_line)
    if s[:2] == b"##":
        return "GFF"                                              # whatever follows
    if s[:1] == b"@":
        return "SAM"
    if s[:1] == b">":
        return None
    n = tc.count_tokens(s, 0x09)
    if n == 1 or 3 <= n <= 6:
        return "BED"
    if n >= 6:
        cur = tc.Cursor(s, 0x09)
        for _ in range(5):
            cur.take()
        sixth = cur.take()
        if b"+" in sixth or b"-" in sixth:
            return "BED"
        if n >= 11:
            return "SAM"
        if 8 <= n <= 10:
            return "GFF"
    return None


# first lines and what the file is: (name, line, format, why)
DETECT = [
    ("score-dot", b"chr1\tsrc\texon\t100\t200\t.\t+\t.\tg1", "GFF", "9 tokens, a sixth token without a sign (:3755)"),
    ("score-decimal", b"chr1\tsrc\texon\t100\t200\t0.5\t-\t0", "GFF", "8 tokens"),
    ("ten-tokens", b"chr1\tsrc\texon\t100\t200\t7\t.\t.\tg1\tnote", "GFF", "10 tokens"),
    ("score-minus", b"chr1\tsrc\texon\t100\t200\t-1.5\t+\t.\tg1", "BED", "a '-' in the sixth token: BED (:3753)"),
    ("score-exponent", b"chr1\tsrc\texon\t100\t200\t1e-5\t+\t.\tg1", "BED", "1e-5 holds a '-': BED"),
    ("score-plus", b"chr1\tsrc\texon\t100\t200\t+3\t+\t.\tg1", "BED", "a '+' in the sixth token"),
    ("eleven-tokens", b"chr1\tsrc\texon\t100\t200\t.\t+\t.\tg1\tnote\tmore", "SAM", "11 tokens are not GFF (:3754)"),
    ("seven-tokens", b"chr1\tsrc\texon\t100\t200\t.\t+", None, "7 tokens: neither"),
    ("header", b"##gff-version 3", "GFF", "a '##' first line: GFF whatever follows (:3725)"),
    ("comment", b"#a comment", "BED", "one '#' is no header: one token reads as BED (:3745)"),
    ("bed6", b"chr1\t99\t200\tg1\t0\t+", "BED", "6 tokens"),
]


# ---------------------------------------------------------------------------------------------------------------------------
# the probes: one line each.  In a template {c} is the chromosome, {s} / {e} START and END of the filler line the probe replaces,
# {ps} the START of the line in front of it (0 at line 0), {cn} / {cp} the known chromosome behind / in front of {c}
# (text_cases.Probe).
# plain: the documented plain case of GTX_TEXT_GFF in include/gtx.h -- where the restatement finds no error, the device must keep
# the block.  (Where the restatement finds one -- a '.' strand in a strand-aware run is never plain -- nothing is claimed.)
# ---------------------------------------------------------------------------------------------------------------------------
BASE = dict(c=b"{c}", src=b"src", ft=b"exon", s=b"{s}", e=b"{e}", sc=b".", st=b"+", fr=b".", lab=b"3", cm=b"note")
COLUMNS = ("c", "src", "ft", "s", "e", "sc", "st", "fr", "lab", "cm")
COLUMN_NAMES = ("seqname", "source", "feature", "START", "END", "score", "strand", "frame", "label", "comment")


def gff(cols=9, tail=b"", **over):
    """the base feature ([{s}, {e}] of {c}, '+', label 3) in `cols` columns with some replaced and `tail` behind all"""
    assert set(over) <= set(BASE)
    f = dict(BASE, **over)
    return b"\t".join(f[k] for k in COLUMNS[:cols]) + tail


def _p(group, name, template, about, plain=False, big=False):
    return Probe(name, template, about, plain, group, big)


_BLANK_INSIDE = dict(c=b"{c} x", src=b"s rc", ft=b"ex on", s=b"{s} 1", e=b"{e} 1", sc=b"0 .5", st=b"+ ", fr=b". ")

PROBES = [
    # token counts (:3504-3505)
    _p("columns", "7-columns", gff(cols=7), "7 tokens: wrong number"),
    _p("columns", "8-columns", gff(cols=8), "8 tokens: the label is _", plain=True),
    _p("columns", "9-columns", gff(cols=9), "9 tokens", plain=True),
    _p("columns", "10-columns", gff(cols=10), "10 tokens", plain=True),
    _p("columns", "11-columns", gff(cols=10, tail=b"\tmore"), "11 tokens: wrong number"),
    _p("columns", "trailing-tab-8", gff(cols=8, tail=b"\t"), "a tab behind the frame: still 8 tokens"),
    _p("columns", "trailing-tab-9", gff(cols=9, tail=b"\t"), "a tab behind the label: still 9 tokens"),
    _p("columns", "trailing-tab-10", gff(cols=10, tail=b"\t"), "a tab behind the comment: still 10 tokens"),
    _p("columns", "one-token", b"{c}", "a line of one token"),
    _p("columns", "empty-line", b"", "an empty line"),
    _p("columns", "comment-line", b"#a comment", "a '#' comment is a data line of one token"),
    _p("columns", "header-line-late", b"##gff-version 3", "a '##' line behind the top of the file is a data line"),
] + [
    _p("columns", "empty-" + COLUMN_NAMES[k], gff(cols=10, **{COLUMNS[k]: b""}), "an empty " + COLUMN_NAMES[k] + " (10 columns written)") for k in range(10)
] + [
    # bytes
    _p("bytes", "blank-inside-" + COLUMN_NAMES[k], gff(**{COLUMNS[k]: _BLANK_INSIDE[COLUMNS[k]]}), "a blank inside " + COLUMN_NAMES[k]) for k in range(8)
] + [
    _p("bytes", "blank-before-" + COLUMN_NAMES[k], gff(cols=10, **{COLUMNS[k]: b" " + BASE[COLUMNS[k]]}), "a blank in front of " + COLUMN_NAMES[k],
       plain=k == 9) for k in range(10)
] + [
    _p("bytes", "blank-comment", gff(cols=10, cm=b"  "), "a comment of blanks alone: 9 tokens", plain=True),
    _p("bytes", "crlf-8", gff(cols=8, tail=b"\r"), "a carriage return behind the frame"),
    _p("bytes", "crlf-9", gff(cols=9, tail=b"\r"), "a carriage return behind the label"),
    _p("bytes", "crlf-10", gff(cols=10, tail=b"\r"), "a carriage return behind the comment"),
    _p("bytes", "cr-inside-label", gff(cols=10, lab=b"3\rx"), "a carriage return inside the label", plain=True),
    _p("bytes", "nul-seqname", gff(c=b"ch\x00r1"), "a NUL in the seqname: the C string is one token"),
    _p("bytes", "nul-feature", gff(ft=b"ex\x00on"), "a NUL in the feature: 3 tokens"),
    _p("bytes", "nul-label", gff(lab=b"3\x004"), "a NUL in the label: it ends there, 9 tokens", plain=True),
    _p("bytes", "nul-label-10", gff(cols=10, lab=b"3\x004"), "the same with a comment behind it: the host sees 9 tokens", plain=True),
    _p("bytes", "nul-label-first", gff(lab=b"\x003"), "a NUL as the label's first byte: the host sees 8 tokens"),
    _p("bytes", "nul-comment", gff(cols=10, cm=b"no\x00te"), "a NUL in the comment", plain=True),
    _p("bytes", "high-byte-seqname", gff(c=b"{c}\xe9"), "a byte >= 0x80 in the seqname: sorts behind every ASCII name", plain=True),
    _p("bytes", "high-byte-label", gff(lab=b"3\xff\x80"), "bytes >= 0x80 in the label", plain=True),
    # START and END (an empty START and an empty END are among the empty columns)
    _p("coord", "start-0", gff(s=b"0"), "START 0", plain=True),
    _p("coord", "start-1", gff(s=b"1"), "START 1", plain=True),
    _p("coord", "end-0", gff(s=b"0", e=b"0"), "END 0: stop 0"),
    _p("coord", "start-above-end", gff(s=b"{e+2}"), "START = END + 2"),
    _p("coord", "zero-length", gff(s=b"{e+1}"), "START = END + 1"),
    _p("coord", "leading-zeros", gff(s=b"00{s}", e=b"000{e}"), "leading zeros", plain=True),
    _p("coord", "start-plus", gff(s=b"+{s}"), "a + sign on START"),
    _p("coord", "start-minus", gff(s=b"-{s}"), "a - sign on START"),
    _p("coord", "end-plus", gff(e=b"+{e}"), "a + sign on END"),
    _p("coord", "end-minus", gff(e=b"-{e}"), "a - sign on END"),
    _p("coord", "start-letter", gff(s=b"{s}x"), "a letter behind START's digits"),
    _p("coord", "end-letter", gff(e=b"{e}x"), "a letter behind END's digits"),
    _p("coord", "start-11-digits-small", gff(s=b"00000000002"), "11 digits that read as 2"),
    _p("coord", "end-11-digits-small", gff(e=b"00000000640"), "11 digits that read as 640"),
    _p("coord", "start-10-digits-small", gff(s=b"0000000002"), "10 digits that read as 2", plain=True),
    _p("coord", "ten-digits-below", gff(s=b"2147483644", e=b"2147483645"), "END 2^31 - 3: the last one kept", plain=True, big=True),
    _p("coord", "ten-digits-start-below", gff(s=b"2147483645", e=b"2147483645"), "START 2^31 - 3", plain=True, big=True),
    _p("coord", "ten-digits-end-at", gff(s=b"2147483644", e=b"2147483646"), "END 2^31 - 2: the 32-bit error", big=True),
    _p("coord", "ten-digits-start-at", gff(s=b"2147483646", e=b"2147483647"), "START 2^31 - 2", big=True),
    _p("coord", "eleven-digits", gff(s=b"10000000000", e=b"10000000001"), "11 digits", big=True),
    # strand: the first byte of column 7, kept raw (:3512)
    _p("strand", "strand-plus", gff(st=b"+"), "strand +", plain=True),
    _p("strand", "strand-minus", gff(st=b"-"), "strand -", plain=True),
    _p("strand", "strand-dot", gff(st=b"."), "strand .: a third strand -- counted when the strand is ignored, else this build's error"),
    _p("strand", "strand-question", gff(st=b"?"), "strand ?"),
    _p("strand", "strand-1", gff(st=b"1"), "strand 1: no BED spelling here"),
    _p("strand", "strand-two-bytes", gff(st=b"+-"), "a strand of two bytes: the first counts"),
    _p("strand", "strand-minus-1", gff(st=b"-1"), "strand -1: the first byte counts"),
    _p("strand", "strand-dot-8", gff(cols=8, st=b"."), "strand . on an 8-column line"),
    # labels (column 9 under max_label > 1)
    _p("label", "label-underscore", gff(lab=b"_"), "_: 0", plain=True),
    _p("label", "label-7", gff(lab=b"7"), "7", plain=True),
    _p("label", "label-7up", gff(lab=b"7up"), "7up", plain=True),
    _p("label", "label--3", gff(lab=b"-3"), "-3", plain=True),
    _p("label", "label-+4", gff(lab=b"+4"), "+4", plain=True),
    _p("label", "label-gtf", gff(lab=b'gene_id "ENSG0001.5"; transcript_id "T 7"; level 2;'), "a GTF attribute string: 0", plain=True),
    _p("label", "label-gtf-10", gff(cols=10, lab=b'gene_id "ENSG0001.5"; level 2;'), "... with a comment behind it", plain=True),
    _p("label", "label-int32-max", gff(lab=b"2147483647"), "2147483647", plain=True),
    _p("label", "label-int32-max+1", gff(lab=b"2147483648"), "2147483648", plain=True),
    _p("label", "label-int32-min", gff(lab=b"-2147483648"), "-2147483648", plain=True),
    _p("label", "label-int32-min-1", gff(lab=b"-2147483649"), "-2147483649: no int32 weight"),
    _p("label", "label-18-digits", gff(lab=b"999999999999999999"), "18 digits", plain=True),
    _p("label", "label-19-digits", gff(lab=b"9999999999999999999"), "19 digits: wraps below zero"),
    _p("label", "label-control-byte", gff(lab=b"\x0b7"), "a vertical tab in front: atol skips it"),
    # chromosomes
    _p("chrom", "unknown-chrom", gff(c=b"chr1_x"), "an unknown chromosome that sorts between chr10 and chr2", plain=True),
    _p("chrom", "unknown-chrom-first", gff(c=b"chr0"), "an unknown chromosome that sorts in front of every known one", plain=True),
    _p("chrom", "prefix-chrom", gff(c=b"chr"), "a proper prefix of every known name", plain=True),
    _p("chrom", "longer-chrom", gff(c=b"{c}0"), "the known name with a 0 behind it", plain=True),
    _p("chrom", "end-0-unknown", gff(c=b"chr1_x", s=b"0", e=b"0"), "stop 0 on an unknown chromosome: dropped before it is validated", plain=True),
    # order
    _p("order", "equal-start", gff(s=b"{ps}"), "the START of the line before", plain=True),
    _p("order", "start-lower-by-1", gff(s=b"{ps-1}"), "one below the START of the line before"),
    _p("order", "chrom-forward", gff(c=b"{cn}"), "the next chromosome early"),
    _p("order", "chrom-backward", gff(c=b"{cp}"), "the chromosome before, again"),
    _p("order", "strand-back", gff(st=b"+"), "strand + (behind - lines, under sorted_by_strand, that is late)", plain=True),
    _p("order", "strand-forward", gff(st=b"-"), "strand - (in front of + lines, under sorted_by_strand, the NEXT line is late)", plain=True),
]
PROBE = {p.name: p for p in PROBES}
assert len(PROBE) == len(PROBES)
ORDER_PROBES = [p for p in PROBES if p.group == "order" and not p.name.startswith("strand-")]


# ---------------------------------------------------------------------------------------------------------------------------
# filler and placements
# ---------------------------------------------------------------------------------------------------------------------------
_FEATURES = ("exon", "CDS", "gene", "start_codon")
_SCORES = (".", "0.5", "12", "1e3")


@functools.lru_cache(maxsize=None)
def filler_line(f, cols=None):
    """the plain feature of one text_cases.filler_fields entry (chromosome, col2, col3, label, strand): START = col2, END = col3,
    column 9 the label (a number, or every fifth line a GTF attribute string led by it); source, feature, score, frame and the column
    count (8, 9 or 10 unless `cols` says) vary with the line"""
    c, s, e, lab, strand = f
    g = s - 2
    cols = 8 + g % 3 if cols is None else cols
    label = str(lab) if g % 5 else '%d gene_id "G%d"; n "a b";' % (lab, g)
    tok = [c, "src%d" % (g % 4), _FEATURES[g % 4], str(s), str(e), _SCORES[g % 4], strand, ".012"[g % 4], label, "note %d" % g]
    return "\t".join(tok[:cols]).encode()


def _pad(line, k):
    """the filler line k bytes longer: more text in its last column (the frame's first byte, the label's number and the comment
    stay what they were)"""
    return line + b"p" * k


def place(probe, j, n_lines, **kw):
    """text_cases.place over GFF filler lines"""
    kw.setdefault("cols", None)
    return tc.place(probe, j, n_lines, filler_line=filler_line, _pad=_pad, **kw)


def stretched(lines, total_bytes):
    return tc.stretched(lines, total_bytes, _pad=_pad)


def long_line(f, size):
    """the filler feature of `f` in `size` bytes, most of them its attribute column"""
    line = filler_line(f, 9)
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
