"""A plain restatement of how a block of BED text becomes packed triples, and the case tables of the tokenizer tests.

Not a test file.  tests/test_text_cases_cpu.py pins `expected` to gtx_packtool (the host packer, csrc/gtx_bed.cpp) and to the
oracle's CLI; tests/test_gpu_text_seams.py then holds the device tokenizer (csrc/gtx_text.hip) to it.  Plain loops only: nothing
here calls into gtx or oracle.

The rules restated (csrc/gtx_bed.cpp: ParseTabbedLine, ParseBedLine, ParsePiece, HandleRecord):
  * a line is cut at tabs when it holds one, else at blanks; blanks in front of a token are skipped; a C string ends at a NUL
  * columns 2, 3 and 4 are read by atol (blanks, a sign, digits, the rest ignored; 64-bit wrap); start = col2 + 1, stop = col3
  * the strand column (the sixth) is one of + . 1 (plus) or - -1 (minus); anything else is an error; 12 columns are an error
  * a coordinate at or above 2^31 - 2 is an error, whatever the chromosome
  * sorted modes (os, ss): the key (name by strcmp on unsigned bytes, [strand,] start) must not sort before the key of the line in
    front of it -- a line dropped for its chromosome counts as such a line, and the check runs on across blocks
  * min(max_label, atol(col4)) (0 without a fourth column) joins the label sum for every line that gets this far
  * a line of an unknown chromosome is dropped before its interval is validated
  * ou: stop <= 0 or start > stop is an error; su: such a line is dropped; os, ss: kept as it is
  * a weight outside int32 is an error
"""
import functools
import random

NAMES = ["chr1", "chr10", "chr2"]          # strcmp order; chr1 is a prefix of chr10
L = 640                                    # filler and probe coordinates stay within 1..L
ERROR = "ERROR"
MODES = ("ou", "os", "su", "ss")

# the kernels' constants (csrc/gtx_text.hip)
K_LINES = 128
K_SEG = 1024
K_LANE = 16
K_TILE = 256
K_LDS_TEXT = 40 * 1024
K_PREV_MAX = 4096

LINE_POSITIONS = (0, 1, 63, 64, 127, 128, 129, 255, 256, 257, "last")
LINE_COUNTS = (1, 2, 127, 128, 129, 256, 257, 300)
NEWLINE_OFFSETS = (15, 16, 1007, 1023, 1024, 1025, 2047, 2048)
LEN_MOD_16 = (0, 1, 15)
LEN_MOD_1024 = (0, 1, 1023)

_U64 = 1 << 64
INT_MAX = 2147483647
INT_MIN = -2147483648


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def c_string(b):
    """the bytes in front of the first NUL"""
    k = b.find(b"\0")
    return b if k < 0 else b[:k]


def atol(tok):
    """FastAtol of csrc/gtx_bed.cpp: blanks and \\t..\\r skipped, an optional sign, digits; unsigned 64-bit wrap, then signed"""
    i, n = 0, len(tok)
    while i < n and (tok[i] == 0x20 or 0x09 <= tok[i] <= 0x0d):
        i += 1
    neg = False
    if i < n and tok[i] in b"+-":
        neg = tok[i] == 0x2d
        i += 1
    v = 0
    while i < n and 0x30 <= tok[i] <= 0x39:
        v = (v * 10 + tok[i] - 0x30) % _U64
        i += 1
    if v >= _U64 // 2:
        v -= _U64
    if neg:
        v = -v
        if v >= _U64 // 2:
            v -= _U64
    return v


def _strand_of(tok):
    if tok in (b"+", b".", b"1"):
        return "+"
    if tok in (b"-", b"-1"):
        return "-"
    return None


def _count_tokens(s, sep):
    i, n, k = 0, len(s), 0
    while i < n and s[i] == 0x20:
        i += 1
    while i < n:
        while i < n and s[i] != sep:
            i += 1
        if i < n:
            i += 1
        k += 1
        while i < n and s[i] == 0x20:
            i += 1
    return k


class _Cursor:
    def __init__(self, s, sep):
        self.s, self.i, self.sep = s, 0, sep

    def take(self):
        s, i = self.s, self.i
        while i < len(s) and s[i] == 0x20:
            i += 1
        e = i
        while e < len(s) and s[e] != self.sep:
            e += 1
        self.i = e + 1 if e < len(s) else e
        return s[i:e]


@functools.lru_cache(maxsize=None)
def read_line(line):
    """One line (without its newline) as the host packer reads it: ERROR, or (name, start, stop, strand, label value)."""
    tabs = [k for k in range(len(line)) if line[k] == 0x09]
    if b" " not in line and len(tabs) >= 2:                       # the one-pass reader of the common shape (ParseTabbedLine)
        n_tokens = len(tabs) + (1 if len(line) > tabs[-1] + 1 else 0)
        cut = [-1] + tabs + [len(line)]
        tok = [line[cut[k] + 1:cut[k + 1]] for k in range(len(cut) - 1)]
        strand = _strand_of(tok[5]) if n_tokens >= 6 else "+"
        if 3 <= n_tokens <= 11 and strand is not None:
            label = atol(c_string(tok[3])) if n_tokens >= 4 else 0
            return _checked(c_string(tok[0]), atol(tok[1]) + 1, atol(tok[2]), strand, label)
    s = c_string(line)                                            # the general reader (ParseBedLine)
    sep = 0x09 if b"\t" in s else 0x20
    n_tokens = _count_tokens(s, sep)
    if n_tokens < 3:
        return ERROR
    cur = _Cursor(s, sep)
    name = cur.take()
    start = atol(cur.take()) + 1
    stop = atol(cur.take())
    label = atol(cur.take()) if n_tokens != 3 else 0
    if n_tokens >= 5:
        cur.take()
    strand = "+"
    if n_tokens >= 6:
        strand = _strand_of(cur.take())
        if strand is None:
            return ERROR
    if n_tokens == 12:
        return ERROR
    return _checked(name, start, stop, strand, label)


def _checked(name, start, stop, strand, label):
    if start >= INT_MAX - 1 or stop >= INT_MAX - 1 or start <= INT_MIN + 1 or stop <= INT_MIN + 1:
        return ERROR
    return name, start, stop, strand, label


def lines_of(block):
    assert block.endswith(b"\n")
    return block[:-1].split(b"\n")


count_tokens, Cursor, checked = _count_tokens, _Cursor, _checked     # (tests/sam_cases.py restates the SAM reader with them)


def seam_key(block, read_line=read_line):
    """(name, strand, start) of the block's last line as the host reads it -- what prev_* of the next block holds -- or None"""
    r = read_line(lines_of(block)[-1])
    return None if r == ERROR else (r[0], r[3], r[1])


def expected_blocks(blocks, mode, names, strand_aware=False, sorted_by_strand=False, max_label=1, prev=None, read_line=read_line):
    """Per block: ERROR, or the list of (class, start, stop, weight) of the lines that are kept, in line order.  Also per block the
    label sum of its lines (None for an ERROR block).  prev: the key (name, strand, start) in front of the first block.
    read_line: the reader of one line (tests/sam_cases.py passes its own; everything behind the reader is the same for SAM)."""
    assert mode in MODES
    names = sorted(n.encode() if isinstance(n, str) else n for n in names)
    sorted_mode = mode in ("os", "ss")
    weighted = max_label > 1
    out, sums = [], []
    for block in blocks:
        kept, total, bad = [], 0, False
        for line in lines_of(block):
            r = read_line(line)
            if r == ERROR:
                bad = True
                break
            name, start, stop, strand, label = r
            if sorted_mode:
                if prev is not None:
                    pname, pstrand, pstart = prev
                    if name != pname:
                        before = name < pname
                    elif sorted_by_strand and strand != pstrand:
                        before = strand < pstrand
                    else:
                        before = start < pstart
                    if before:
                        bad = True
                        break
                prev = (name, strand, start)
            w = min(label, max_label) if weighted else 1
            total += w
            if name not in names:
                continue
            if mode == "ou" and (stop <= 0 or start > stop):
                bad = True
                break
            if mode == "su" and (start > stop or stop <= 0):
                continue
            if w > INT_MAX or w < INT_MIN:
                bad = True
                break
            cls = names.index(name) + (len(names) if strand_aware and strand == "-" else 0)
            kept.append((cls, start, stop, w))
        if bad:
            out.append(ERROR)
            sums.append(None)
            if sorted_mode:                                       # the next block's seam key is its last line's, as the caller fills it
                k = seam_key(block, read_line)
                prev = k if k is not None else prev
        else:
            out.append(kept)
            sums.append(total)
    return out, sums


def expected(blocks, mode, names, strand_aware=False, sorted_by_strand=False, max_label=1, prev=None):
    """(per block ERROR or its kept (class, start, stop, weight), the label sum over the blocks without an error)"""
    out, sums = expected_blocks(blocks, mode, names, strand_aware, sorted_by_strand, max_label, prev)
    return out, sum(s for s in sums if s is not None)


def grouped(kept, n_chrom):
    """the order the host packer hands a strand-aware batch over in: the '+' reads, then the '-' reads, each in line order"""
    return [k for k in kept if k[0] < n_chrom] + [k for k in kept if k[0] >= n_chrom]


def depth(kept_lists, n_classes, length=L, lo=1):
    """weighted depth per (class, base lo..lo+length-1) of the kept lines, modulo 2^64: what a count over unit-width regions returns
    (every line adds its weight at its first base and takes it back behind its last; a running sum per class)"""
    step = [0] * (n_classes * (length + 1))
    for kept in kept_lists:
        for cls, start, stop, w in kept:
            a, b = max(start, lo), min(stop, lo + length - 1)
            if a <= b:
                step[cls * (length + 1) + a - lo] += w
                step[cls * (length + 1) + b - lo + 1] -= w
    out = []
    for c in range(n_classes):
        run = 0
        for k in range(length):
            run += step[c * (length + 1) + k]
            out.append(run % _U64)
    return out


def unit_refs(n_classes, length=L, lo=1):
    return [(c, p, p) for c in range(n_classes) for p in range(lo, lo + length)]


# ---------------------------------------------------------------------------------------------------------------------------
# the probes: one line each.  In a template {c} {s} {e} are the chromosome, column 2 and column 3 of the filler line the probe
# replaces, {ps} column 2 of the line in front of it (0 at line 0), {cn} / {cp} the known chromosome behind / in front of {c}.
# plain: the documented plain case of include/gtx.h -- where the restatement finds no error, the device must keep the block.
# ---------------------------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, name, template, about, plain=False, group="", big=False):
        self.name, self.template, self.about, self.plain, self.group, self.big = name, template, about, plain, group, big

    def line(self, c="chr1", s=100, e=110, ps=99):
        k = NAMES.index(c)
        f = {b"{c}": c, b"{s}": s, b"{e}": e, b"{ps}": ps, b"{ps-1}": ps - 1, b"{e+1}": e + 1, b"{e+2}": e + 2,
             b"{cn}": NAMES[min(k + 1, len(NAMES) - 1)], b"{cp}": NAMES[max(k - 1, 0)]}
        out = self.template
        for key, v in f.items():
            out = out.replace(key, str(v).encode())
        assert b"\n" not in out
        return out

    def __repr__(self):
        return self.name


def _p(group, name, template, about, plain=False, big=False):
    return Probe(name, template, about, plain, group, big)


PROBES = [
    # separators and line shape
    _p("shape", "blanks", b"{c} {s} {e} 3 0 +", "a space-separated line"),
    _p("shape", "empty-token", b"{c}\t{s}\t{e}\t\t0\t+", "an empty fourth token"),
    _p("shape", "trailing-tab", b"{c}\t{s}\t{e}\t", "a tab behind the third column"),
    _p("shape", "crlf", b"{c}\t{s}\t{e}\r", "a carriage return in front of the newline"),
    _p("shape", "empty-line", b"", "an empty line"),
    _p("shape", "lone-name", b"{c}", "a name and nothing else"),
    _p("shape", "two-columns", b"{c}\t{s}", "two columns"),
    # coordinate columns
    _p("coord", "plus-col2", b"{c}\t+{s}\t{e}", "a + sign on column 2"),
    _p("coord", "minus-col2", b"{c}\t-{s}\t{e}", "a - sign on column 2"),
    _p("coord", "plus-col3", b"{c}\t{s}\t+{e}", "a + sign on column 3"),
    _p("coord", "minus-col3", b"{c}\t{s}\t-{e}", "a - sign on column 3"),
    _p("coord", "leading-zeros", b"{c}\t00{s}\t000{e}", "leading zeros"),
    _p("coord", "ten-digits-below", b"{c}\t2147483643\t2147483644", "10 digits just below the limit: kept", plain=True, big=True),
    _p("coord", "ten-digits-at", b"{c}\t2147483645\t2147483646", "10 digits at the limit: the 32-bit error", big=True),
    _p("coord", "ten-digits-col3-at", b"{c}\t{s}\t2147483646", "column 3 at the limit", big=True),
    _p("coord", "eleven-digits", b"{c}\t10000000000\t10000000001", "11 digits", big=True),
    _p("coord", "eleven-digits-col3", b"{c}\t{s}\t00000000{e}", "11 digits that read as a small number"),
    # column counts
    _p("columns", "3-columns", b"{c}\t{s}\t{e}", "3 columns", plain=True),
    _p("columns", "4-columns", b"{c}\t{s}\t{e}\t4", "4 columns", plain=True),
    _p("columns", "5-columns", b"{c}\t{s}\t{e}\t4\t0", "5 columns", plain=True),
    _p("columns", "6-columns", b"{c}\t{s}\t{e}\t4\t0\t-", "6 columns", plain=True),
    _p("columns", "7-columns", b"{c}\t{s}\t{e}\t4\t0\t-\tx", "7 columns", plain=True),
    _p("columns", "11-columns", b"{c}\t{s}\t{e}\t4\t0\t-\t1\t2\t3\t4\t5", "11 columns", plain=True),
    _p("columns", "12-columns", b"{c}\t{s}\t{e}\t4\t0\t+\t{s}\t{e}\t0\t1\t5,\t0,", "12 columns: BED12"),
    _p("columns", "13-columns", b"{c}\t{s}\t{e}\t4\t0\t+\t{s}\t{e}\t0\t1\t5,\t0,\tx", "13 columns"),
    # strand tokens
    _p("strand", "strand-plus", b"{c}\t{s}\t{e}\t4\t0\t+", "strand +", plain=True),
    _p("strand", "strand-minus", b"{c}\t{s}\t{e}\t4\t0\t-", "strand -", plain=True),
    _p("strand", "strand-dot", b"{c}\t{s}\t{e}\t4\t0\t.", "strand .", plain=True),
    _p("strand", "strand-1", b"{c}\t{s}\t{e}\t4\t0\t1", "strand 1", plain=True),
    _p("strand", "strand--1", b"{c}\t{s}\t{e}\t4\t0\t-1", "strand -1", plain=True),
    _p("strand", "strand-x", b"{c}\t{s}\t{e}\t4\t0\tx", "strand x"),
    _p("strand", "strand-+-", b"{c}\t{s}\t{e}\t4\t0\t+-", "strand +-"),
    _p("strand", "strand---", b"{c}\t{s}\t{e}\t4\t0\t--", "strand --"),
    # labels
    _p("label", "label-7up", b"{c}\t{s}\t{e}\t7up", "label 7up", plain=True),
    _p("label", "label--3", b"{c}\t{s}\t{e}\t-3", "label -3", plain=True),
    _p("label", "label-+4", b"{c}\t{s}\t{e}\t+4", "label +4", plain=True),
    _p("label", "label-blank-5", b"{c}\t{s}\t{e}\t 5", "label ' 5'"),
    _p("label", "label-word", b"{c}\t{s}\t{e}\tname", "a label without digits", plain=True),
    _p("label", "label-18-digits", b"{c}\t{s}\t{e}\t999999999999999999", "18 digits", plain=True),
    _p("label", "label-19-digits", b"{c}\t{s}\t{e}\t9999999999999999999", "19 digits: wraps below zero"),
    _p("label", "label-int32-max", b"{c}\t{s}\t{e}\t2147483647", "2147483647", plain=True),
    _p("label", "label-int32-max+1", b"{c}\t{s}\t{e}\t2147483648", "2147483648", plain=True),
    _p("label", "label-int32-min", b"{c}\t{s}\t{e}\t-2147483648", "-2147483648", plain=True),
    _p("label", "label-int32-min-1", b"{c}\t{s}\t{e}\t-2147483649", "-2147483649: no int32 weight"),
    _p("label", "label--5e9", b"{c}\t{s}\t{e}\t-5000000000", "-5000000000: no int32 weight"),
    # bytes
    _p("bytes", "high-byte-name", b"{c}\xe9\t{s}\t{e}", "a byte >= 0x80 in the name"),
    _p("bytes", "high-byte-label", b"{c}\t{s}\t{e}\t3\xff\x80", "bytes >= 0x80 in the label"),
    _p("bytes", "nul-name", b"ch\0r1\t{s}\t{e}", "a NUL in the name"),
    _p("bytes", "nul-label", b"{c}\t{s}\t{e}\t3\x004", "a NUL in the label"),
    # chromosome names
    _p("chrom", "unknown-chrom", b"chr1_x\t{s}\t{e}", "an unknown chromosome that sorts between chr10 and chr2", plain=True),
    _p("chrom", "unknown-chrom-late", b"chr0\t{s}\t{e}", "an unknown chromosome that sorts in front of every known one", plain=True),
    _p("chrom", "prefix-chrom", b"chr\t{s}\t{e}", "a proper prefix of every known name", plain=True),
    _p("chrom", "longer-chrom", b"{c}0\t{s}\t{e}", "the known name with a 0 behind it", plain=True),
    # intervals
    _p("interval", "stop-0", b"{c}\t0\t0", "stop 0"),
    _p("interval", "start-above-stop", b"{c}\t{e+1}\t{e}", "start > stop (start = stop + 2)"),
    _p("interval", "zero-length", b"{c}\t{e}\t{e}", "start == stop + 1"),
    _p("interval", "stop-0-unknown", b"chr1_x\t0\t0", "stop 0 on an unknown chromosome"),
    _p("interval", "start-above-stop-unknown", b"chr1_x\t{e+1}\t{e}", "start > stop on an unknown chromosome"),
    _p("interval", "zero-length-unknown", b"chr1_x\t{e}\t{e}", "start == stop + 1 on an unknown chromosome"),
    # order
    _p("order", "equal-start", b"{c}\t{ps}\t{e}\t4\t0\t+", "the start of the line before", plain=True),
    _p("order", "start-lower-by-1", b"{c}\t{ps-1}\t{e}\t4\t0\t+", "one below the start of the line before"),
    _p("order", "chrom-forward", b"{cn}\t{s}\t{e}\t4\t0\t+", "the next chromosome early"),
    _p("order", "chrom-backward", b"{cp}\t{s}\t{e}\t4\t0\t+", "the chromosome before, again"),
    _p("order", "strand-back", b"{c}\t{s}\t{e}\t4\t0\t+", "strand + (behind - lines, under sorted_by_strand, that is late)", plain=True),
]
PROBE = {p.name: p for p in PROBES}
assert len(PROBE) == len(PROBES)
ORDER_PROBES = [p for p in PROBES if p.group == "order" and p.name != "strand-back"]


# ---------------------------------------------------------------------------------------------------------------------------
# filler and placements
# ---------------------------------------------------------------------------------------------------------------------------
def filler_fields(n, first=0, total=None, strands=None):
    """(chromosome, col2, col3, label, strand) of n clean lines: lines first..first+n-1 of a stream of `total` lines in ascending
    order -- the chromosomes in equal shares, col2 = 2 + the line's index in the stream, and within a chromosome the '+' lines in
    front of the '-' lines (in order with and without sorted_by_strand).  strands(i): another strand for line i of the stream."""
    total = n + first if total is None else total
    assert total + 30 < L
    out = []
    for g in range(first, first + n):
        k = g * len(NAMES) // total
        lo, hi = -(-k * total // len(NAMES)), -(-(k + 1) * total // len(NAMES))      # the chromosome's lines: [lo, hi)
        strand = "+" if g - lo < (hi - lo + 1) // 2 else "-"
        if strands is not None:
            strand = strands(g)
        out.append((NAMES[k], 2 + g, 2 + g + 3 + g % 11, g % 7, strand))
    return out


def filler_line(f, cols=7):
    c, s, e, lab, strand = f
    return "\t".join([c, str(s), str(e), str(lab), "0", strand, "p"][:cols]).encode()


def _pad(line, k):
    """the filler line k bytes longer: more text in its last column (column 7; with fewer columns, column 4's digits grow in front)"""
    if k == 0:
        return line
    tok = line.split(b"\t")
    assert len(tok) in (4, 7)
    tok[-1] = tok[-1] + b"p" * k if len(tok) == 7 else b"0" * k + tok[-1]
    return b"\t".join(tok)


def place(probe, j, n_lines, first_byte=None, total_bytes_mod=None, newline_at=None, cols=7, first=0, total=None, strands=None,
          extra=None, stretch=None, filler_line=filler_line, _pad=_pad):
    """A block of n_lines clean ascending filler lines with the probe (a Probe, bytes, or None for none) at line j ("last": the last
    line).  first_byte: the probe's first byte lands on that offset of the block; newline_at: its newline does;
    total_bytes_mod = (m, r): len(block) % m == r.  The lines in front of the probe (and the last line) grow to make it so.
    extra: {line: Probe or bytes} more lines replaced; stretch: {line: length} filler lines grown to that many bytes.
    filler_line, _pad: how a filler line is written and grown (tests/sam_cases.py passes its own)."""
    if j == "last":
        j = n_lines - 1
    assert 0 <= j < n_lines
    fields = filler_fields(n_lines, first, total, strands)
    lines = [filler_line(f, cols) for f in fields]
    for k, what in [(j, probe)] + sorted((extra or {}).items()):
        if what is not None:
            c, s, e = fields[k][:3]
            lines[k] = what.line(c, s, e, fields[k - 1][1] if k else 0) if isinstance(what, Probe) else what
    for k, size in (stretch or {}).items():
        lines[k] = _pad(lines[k], size - len(lines[k]))
    if newline_at is not None:
        assert first_byte is None
        first_byte = newline_at - len(lines[j])
    pad_for_total = n_lines - 1 if j != n_lines - 1 else j - 1
    if first_byte is not None:
        assert j >= 1
        need = first_byte - sum(len(l) + 1 for l in lines[:j])
        assert need >= 0, "the lines in front of the probe are already longer than that"
        per, rest = divmod(need, j)                               # spread over the lines in front (a parse block's text must fit LDS)
        for k in range(j):
            lines[k] = _pad(lines[k], per + (rest if k == j - 1 else 0))
        if pad_for_total == j - 1:
            pad_for_total = j - 2
    if total_bytes_mod is not None:
        m, r = total_bytes_mod
        assert pad_for_total >= 0
        have = sum(len(l) + 1 for l in lines)
        lines[pad_for_total] = _pad(lines[pad_for_total], (r - have) % m)
    block = b"\n".join(lines) + b"\n"
    if first_byte is not None:
        assert sum(len(l) + 1 for l in lines[:j]) == first_byte
    if total_bytes_mod is not None:
        assert len(block) % total_bytes_mod[0] == total_bytes_mod[1]
    return block


def stretched(lines, total_bytes, _pad=_pad):
    """the filler lines grown evenly until they and their newlines are total_bytes long"""
    need = total_bytes - sum(len(l) + 1 for l in lines)
    assert need >= 0
    per, rest = divmod(need, len(lines))
    return [_pad(l, per + (1 if k < rest else 0)) for k, l in enumerate(lines)]


# ---------------------------------------------------------------------------------------------------------------------------
# the fuzz generator
# ---------------------------------------------------------------------------------------------------------------------------
def fuzz_blocks(seed, n_blocks, probes=None):
    """n_blocks independent blocks of 1..400 lines: every even-numbered block clean, every other one with exactly one line replaced
    by a random probe at a random line.  Returns [(block, probe or None, line)]."""
    rng = random.Random(seed)
    probes = [p for p in PROBES if not p.big] if probes is None else probes
    out = []
    for b in range(n_blocks):
        n = rng.randint(1, 400)
        if b % 2 == 0:
            out.append((place(None, 0, n), None, -1))
        else:
            p, j = rng.choice(probes), rng.randrange(n)
            out.append((place(p, j, n), p, j))
    return out
