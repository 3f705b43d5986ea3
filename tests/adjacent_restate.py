"""`genomic_regions test | gdist | inv` restated in Python -- TEST INFRASTRUCTURE ONLY: the yardstick of the genomic_adjacent tests.

The three loops are the reference's, written as they stand in gtools/genomic_intervals.cpp.  All compare a region r with the one
directly in front of it, r0 (never a running maximum), on the front intervals:
  * IsBefore (:396-401): chromosome by strcmp, strand only when sorted_by_strand, then START;
  * IsCompatibleWith (:416-421): same chromosome, and same strand unless ignore_strand.

test [-s] (RunGlobalTest :4755-4778): every region must be IsCompatibleSortedAndNonoverlapping (:1153-1161; multi-interval regions
are allowed), else "input regions must be compatible, sorted and non-overlapping!"; then IsBefore(r, r0, sorted_by_strand) is the
order error; then, when compatible (strand ignored without -s), START <= r0.STOP counts an inclusion if STOP <= r0.STOP and an
overlap otherwise.  At the end, on stderr: "* The file is sorted! Found %ld inclusions and %ld overlaps.\\n".

gdist [-op1 X] [-op2 Y] (RunGlobalCalcDistances :4523-4542), sorted_by_strand = true: single-interval check ("this operation requires
single-interval regions!"), order check, then "LABEL(r0) TAB LABEL(r) TAB", then r.GetCoordinate(op2) - r0.GetCoordinate(op1)
(:438-441, :465-472) when chromosome AND strand agree, else "NaN", then the newline.  An unknown operation word is noticed only inside
GetCoordinate, i.e. at the first compatible pair, after the two labels: "Error: unknown offset reference point operation!\\n", exit 1.

inv -g GENOME (RunGlobalInvert :4576-4600), sorted_by_strand = true: the head r0 of a run is checked for a single interval ("not a
single-interval region!") and for its chromosome's bound -- "Line %ld: chromosome %s not found!\\n" with the BUFFER's line counter,
which after the head's construction (:2115-2121) stands on the line behind the head's, or is 0 when the head was the last line
(core.cpp:241-259) -- and prints [1, START - 1] when START > 1; every following region compatible with its predecessor is checked
for a single interval, then for START < r0.START (the order error), and prints [r0.STOP + 1, START - 1] when START > r0.STOP + 1;
the run's last region prints [STOP + 1, size] when STOP + 1 < size.  A gap prints through GenomicRegionBED::PrintModified (:2310-2314):
CHROM TAB start - 1 TAB stop TAB _ TAB score TAB STRAND, score and strand those of the region it is printed through (score 0 for a
line with fewer than 5 tokens, where the reference leaves it unset).

PrintError (:1001-1006) writes "\\nError: Line N: msg\\n" and exits 1; stdout holds what was printed before.  Header lines are echoed.
BED parsing is oracle/restate.py's (1-based inclusive coordinates: BED start + 1).

adjacent_packed / gaps_packed are the same loops on packed (class, start, stop) triples: what the C ABI's gtx_adjacent / gtx_gaps are
held to.
"""
import numpy as np

from oracle import restate

POINTS = {"1": 0, "2": 1, "5p": 2, "3p": 3}
NO_DISTANCE = -2 ** 63


def is_header(line):
    return line.startswith("browser ") or line.startswith("track ")


def is_before(a, b, sorted_by_strand):
    ca, cb = a["chrom"].encode(), b["chrom"].encode()
    if ca != cb:
        return ca < cb
    if sorted_by_strand and a["strand"] != b["strand"]:
        return a["strand"] < b["strand"]
    return a["iv"][0][0] < b["iv"][0][0]


def is_compatible(a, b, ignore_strand):
    return a["chrom"] == b["chrom"] and (ignore_strand or a["strand"] == b["strand"])


def coordinate(start, stop, minus, op):
    """GenomicInterval::GetCoordinate (:465-472); None for an unknown word"""
    if op == "1":
        return start
    if op == "2":
        return stop
    if op == "5p":
        return stop if minus else start
    if op == "3p":
        return start if minus else stop
    return None


def _read(lines):
    out, at = [], 0
    while at < len(lines) and is_header(lines[at]):
        out.append(lines[at] + "\n")
        at += 1
    return out, [(k + 1, restate.parse(lines[k])) for k in range(at, len(lines)) if lines[k] != ""]


def _order_msg(sorted_by_strand):
    return "input regions are not sorted (sorted-by-strand = %s)!" % ("true" if sorted_by_strand else "false")


def _fail(out, n_line, msg):
    return "".join(out), "\nError: Line %d: %s\n" % (n_line, msg), 1


def test_lines(lines, sorted_by_strand=False):
    """(stdout, stderr, exit code) of `genomic_regions test [-s]` on the lines of a BED file (no newlines)"""
    out, regs = _read(lines)
    if not regs:
        return "".join(out), "", 0
    n_inclusions = n_overlaps = 0
    r0 = None
    for n, r in regs:
        if not restate.sorted_disjoint(r["iv"]):
            return _fail(out, n, "input regions must be compatible, sorted and non-overlapping!")
        if r0 is not None:
            if is_before(r, r0, sorted_by_strand):
                return _fail(out, n, _order_msg(sorted_by_strand))
            if is_compatible(r, r0, not sorted_by_strand) and r["iv"][0][0] <= r0["iv"][0][1]:
                if r["iv"][0][1] <= r0["iv"][0][1]:
                    n_inclusions += 1
                else:
                    n_overlaps += 1
        r0 = r
    return "".join(out), "* The file is sorted! Found %d inclusions and %d overlaps.\n" % (n_inclusions, n_overlaps), 0


test_lines.__test__ = False      # (not a test of its own, whatever its name says to pytest)


def gdist_lines(lines, op1="1", op2="1"):
    """(stdout, stderr, exit code) of `genomic_regions gdist -op1 X -op2 Y`"""
    out, regs = _read(lines)
    r0 = None
    for n, r in regs:
        if len(r["iv"]) != 1:
            return _fail(out, n, "this operation requires single-interval regions!")
        if r0 is not None:
            if is_before(r, r0, True):
                return _fail(out, n, _order_msg(True))
            line = "%s\t%s\t" % (r0["label"], r["label"])
            if is_compatible(r, r0, False):
                a = coordinate(r["iv"][0][0], r["iv"][0][1], r["minus"], op2)
                b = coordinate(r0["iv"][0][0], r0["iv"][0][1], r0["minus"], op1)
                if a is None or b is None:
                    return "".join(out) + line, "Error: unknown offset reference point operation!\n", 1
                line += "%d" % (a - b)
            else:
                line += "NaN"
            out.append(line + "\n")
        r0 = r
    return "".join(out), "", 0


def inv_lines(lines, bounds):
    """(stdout, stderr, exit code) of `genomic_regions inv -g GENOME`; bounds: chromosome -> size"""
    out, regs = _read(lines)

    def gap(r, start, stop):
        out.append("%s\t%d\t%d\t_\t%d\t%s\n" % (r["chrom"], start - 1, stop, r["score"], r["strand"]))

    i = 0
    while i < len(regs):
        n0, r0 = regs[i]
        if len(r0["iv"]) != 1:
            return _fail(out, n0, "not a single-interval region!")
        if r0["chrom"] not in bounds:
            return "".join(out), "Line %d: chromosome %s not found!\n" % (n0 + 1 if n0 < len(lines) else 0, r0["chrom"]), 1
        size = bounds[r0["chrom"]]
        if r0["iv"][0][0] > 1:
            gap(r0, 1, r0["iv"][0][0] - 1)
        i += 1
        while i < len(regs) and is_compatible(regs[i][1], r0, False):
            n, r = regs[i]
            if len(r["iv"]) != 1:
                return _fail(out, n, "not a single-interval region!")
            if is_before(r, r0, True):
                return _fail(out, n, _order_msg(True))
            if r["iv"][0][0] > r0["iv"][0][1] + 1:
                gap(r, r0["iv"][0][1] + 1, r["iv"][0][0] - 1)
            r0 = r
            i += 1
        if r0["iv"][0][1] + 1 < size:
            gap(r0, r0["iv"][0][1] + 1, size)
    return "".join(out), "", 0


# ---- the loops on packed triples ----

def adjacent_packed(tri, minus=None, op1=0, op2=0):
    """(distances int64, first_unsorted, n_inclusions, n_overlaps) of gtx_adjacent: the counts cover every same-class neighbour pair of
    the input; distances[i] = coord(i, op2) - coord(i - 1, op1) in the predecessor's class, INT64_MIN otherwise and for row 0"""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    n = len(tri)
    c, s, e = tri[:, 0].tolist(), tri[:, 1].tolist(), tri[:, 2].tolist()
    m = [0] * n if minus is None else [int(x) for x in minus]
    words = ["1", "2", "5p", "3p"]
    dist = [NO_DISTANCE] * n
    first_unsorted, n_inclusions, n_overlaps = -1, 0, 0
    for i in range(1, n):
        if first_unsorted < 0 and (c[i], s[i]) < (c[i - 1], s[i - 1]):
            first_unsorted = i
        if c[i] != c[i - 1]:
            continue
        if s[i] <= e[i - 1]:
            if e[i] <= e[i - 1]:
                n_inclusions += 1
            else:
                n_overlaps += 1
        dist[i] = coordinate(s[i], e[i], m[i], words[op2]) - coordinate(s[i - 1], e[i - 1], m[i - 1], words[op1])
    return np.array(dist, dtype=np.int64), first_unsorted, n_inclusions, n_overlaps


def gaps_packed(tri, bounds):
    """(owners uint32, starts int32, stops int32, first_bad, bad_kind) of gtx_gaps: RunGlobalInvert's loop, stopped in front of the
    first bad row (1: inside a run and before its predecessor; 2: the head of a run whose class has no bound)"""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    n = len(tri)
    c, s, e = tri[:, 0].tolist(), tri[:, 1].tolist(), tri[:, 2].tolist()
    b = [int(x) for x in bounds]
    owners, starts, stops = [], [], []

    def done(first_bad, kind):
        return np.array(owners, dtype=np.uint32), np.array(starts, dtype=np.int32), np.array(stops, dtype=np.int32), first_bad, kind

    i = 0
    while i < n:
        if not (0 <= c[i] < len(b)) or b[c[i]] < 0:
            return done(i, 2)
        size = b[c[i]]
        if s[i] > 1:
            owners.append(i); starts.append(1); stops.append(s[i] - 1)
        i += 1
        while i < n and c[i] == c[i - 1]:
            if s[i] < s[i - 1]:
                return done(i, 1)
            if s[i] > e[i - 1] + 1:
                owners.append(i); starts.append(e[i - 1] + 1); stops.append(s[i] - 1)
            i += 1
        if e[i - 1] + 1 < size:
            owners.append(i - 1); starts.append(e[i - 1] + 1); stops.append(size)
    return done(-1, 0)
