"""Restatement in Python of `genomic_regions shift | shiftp | pos | center | fix | bounds` on BED input, from the reference's source
(file:line of gtools/genomic_intervals.cpp unless said otherwise): the reader (GenomicRegionBED::Read :2157-2182 over CountTokens /
GetNextToken core.cpp:577-625 and ProcessStrand :5956-5962), the operations as GenomicRegionBED's members apply them (:2340-2480 over
GenomicInterval::ShiftPos :524-531, ModifyPos :537-550, ApplyBounds :556-570, GenomicRegion::Center :1293-1301, Fix :1419-1425,
Union :1649-1671, UpdateThick :2326-2333), GenomicRegionBED::Print (:2188-2218), the set's header echo (:3713-3720) and the drivers'
loops (:3954-4140).  All arithmetic is signed and division truncates toward zero, as in C++.  Also the device path's notion of a
plain line (include/gtx.h, gtx_rewrite_text), so that a generator of plain lines can be confirmed on the CPU."""
import re

KINDS = ("shift", "shiftp", "pos", "center", "fix", "bounds")
POS_OPS = ("1", "2", "5p", "3p", "c")


class InputError(Exception):
    def __init__(self, text):
        Exception.__init__(self, text)
        self.text = text


def tdiv(a, b):
    """a / b of C++ on signed integers"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def atol(s):
    m = re.match(r"[ \t\n\v\f\r]*([+-]?)(\d*)", s)
    v = int(m.group(2)) if m.group(2) else 0
    return -v if m.group(1) == "-" else v


def count_tokens(s, delim):
    """CountTokens core.cpp:577-593"""
    k = 0
    while k < len(s) and s[k] == " ":
        k += 1
    n = 0
    while True:
        if k >= len(s):
            return n
        while k < len(s) and s[k] != delim:
            k += 1
        if k < len(s):
            k += 1
        n += 1
        while k < len(s) and s[k] == " ":
            k += 1
        if k >= len(s):
            return n


class Tokens:
    """GetNextToken core.cpp:610-625 over one buffer"""

    def __init__(self, s):
        self.s = s

    def next(self, delim):
        s = self.s.lstrip(" ")
        k = s.find(delim)
        if k < 0:
            self.s = ""
            return s
        self.s = s[k + 1:]
        return s[:k]


def read_bed(line, n_line):
    """GenomicRegionBED::Read :2157-2182: a dict with chrom, strand, n_tokens, label, score, thick, rgb and iv = [[start, stop], ..]"""
    sep = "\t" if "\t" in line else " "
    nt = count_tokens(line, sep)
    if nt < 3:
        raise InputError("\nError: Line %d: number of tokens should be at least 3 for BED format!\n" % n_line)
    t = Tokens(line)
    r = {"n_line": n_line, "n_tokens": nt, "chrom": t.next(sep)}
    start = atol(t.next(sep)) + 1
    stop = atol(t.next(sep))
    r["strand"] = "+"
    r["label"] = "_" if nt == 3 else t.next(sep)
    r["score"] = atol(t.next(sep)) if nt >= 5 else 0
    if nt >= 6:
        w = t.next(sep)
        if w in ("1", "+", "."):
            r["strand"] = "+"
        elif w in ("-1", "-"):
            r["strand"] = "-"
        else:
            raise InputError("Error: invalid strand '%s'!\n" % w)
    r["thick"] = [0, 0]
    if nt >= 8:
        r["thick"] = [atol(t.next(sep)), atol(t.next(sep))]
    r["rgb"] = t.next(sep) if nt >= 9 else ""
    if nt != 12:
        r["iv"] = [[start, stop]]
        return r
    n = atol(t.next(sep))
    iv = [[start, stop] for _ in range(n)]
    sizes = Tokens(t.next(sep))
    for i in iv:
        i[1] = atol(sizes.next(","))
    starts = Tokens(t.next(sep))
    for i in iv:
        i[0] += atol(starts.next(","))
        i[1] += i[0] - 1
    r["iv"] = iv
    return r


def union(r):
    """:1649-1671 (the intervals of a BED region share chromosome and strand)"""
    iv = r["iv"]
    if len(iv) <= 1:
        return
    iv.sort(key=lambda i: i[0])
    out = []
    start, stop = iv[0]
    for s, e in iv[1:]:
        if stop < s:
            out.append([start, stop])
            start, stop = s, e
        else:
            stop = max(stop, e)
    out.append([start, stop])
    r["iv"] = out


def fix(r):
    """:1419-1425 with CheckValid :333-338"""
    r["iv"] = [i for i in r["iv"] if not (i[0] < 1 or i[0] > i[1])]


def update_thick(r):
    """:2326-2333"""
    if r["iv"]:
        t = r["thick"]
        t[0] = max(t[0], r["iv"][0][0] - 1)
        t[1] = min(t[1], r["iv"][-1][1])
        if t[1] <= t[0]:
            t[0] = t[1] = r["iv"][0][0] - 1


def apply(op, r):
    """the operation on a region; False: the driver prints nothing for it (RunBounds :3959)"""
    kind = op["kind"]
    if kind in ("shift", "shiftp"):                                   # :2470-2476 over :524-531
        a, b = op["a"], op["b"]
        for i in r["iv"]:
            if kind == "shiftp" and r["strand"] == "-":
                i[0] -= b
                i[1] -= a
            else:
                i[0] += a
                i[1] += b
        union(r)
        update_thick(r)
    elif kind == "pos":                                               # :2437-2442 over :537-550
        w, k = op["op"], op["c"]
        for i in r["iv"]:
            if w == "c":
                m = i[0] + tdiv(i[1] - i[0] + 1, 2)
                i[0], i[1] = m - k, m + k
            else:
                choose_start = w == "1" or (r["strand"] == "+" and w == "5p") or (r["strand"] == "-" and w == "3p")
                if choose_start:
                    i[1] = i[0] + k
                else:
                    i[0] = i[1] - k
        union(r)
    elif kind == "center":                                            # :2357-2362 over :1293-1301
        for i in r["iv"]:
            h = tdiv(i[1] - i[0], 2)
            i[0], i[1] = i[0] + h, i[1] - h
        update_thick(r)
    elif kind == "fix":                                               # :2416-2421
        fix(r)
        update_thick(r)
    elif kind == "bounds":                                            # :3959, :2346-2352 over :1280-1287 and :556-570
        g = op["genome"]
        if r["chrom"] not in g:
            return False
        n = g[r["chrom"]]
        for i in r["iv"]:
            if i[0] > n or i[1] < 1 or i[1] < i[0]:
                i[0] = i[1] = 0
            elif i[0] < 1 or i[1] > n:
                i[0], i[1] = max(i[0], 1), min(i[1], n)
        fix(r)
        update_thick(r)
    else:
        raise ValueError(kind)
    return True


def render(r):
    """GenomicRegionBED::Print :2188-2218; raises InputError with the line printed so far in .partial when exons overlap (:2207)"""
    iv = r["iv"]
    if not iv:
        return ""
    nt = r["n_tokens"]
    out = "%s\t%d\t%d" % (r["chrom"], iv[0][0] - 1, iv[-1][1])
    if nt >= 4:
        out += "\t" + r["label"]
        if nt >= 5:
            out += "\t%d" % r["score"]
            if nt >= 6:
                out += "\t" + r["strand"]
                if nt >= 8:
                    out += "\t%d\t%d" % tuple(r["thick"])
                    if nt >= 9:
                        out += "\t" + r["rgb"]
                        if nt == 12:
                            out += "\t%d\t" % len(iv) + ",".join("%d" % (e - s + 1) for s, e in iv) + "\t0"
                            for j in range(1, len(iv)):
                                if iv[j][0] <= iv[j - 1][1]:
                                    err = InputError("Line %d: exons cannot overlap!\n" % r["n_line"])
                                    err.partial = out
                                    raise err
                                out += ",%d" % (iv[j][0] - iv[0][0])
    return out + "\n"


def is_header(line):
    return line.startswith("browser ") or line.startswith("track ")


def run(op, text):
    """(stdout, stderr, exit status) of the operation on the text of a BED file; only complete lines count (core.cpp:241-259)"""
    lines = text.split("\n")[:-1]
    out = ""
    k = 0
    while k < len(lines) and is_header(lines[k]):                     # :3713-3720, hide_header = false (genomic_regions.cpp:702-704)
        out += lines[k] + "\n"
        k += 1
    if op["kind"] == "pos" and op["op"] not in POS_OPS:               # (the set is open and its header out before RunModifyPos refuses the word, :4081)
        return out, "Error: unknown operation!\n", 1
    for n in range(k, len(lines)):
        try:
            r = read_bed(lines[n], n + 1)
            if apply(op, r):
                out += render(r)
        except InputError as err:
            return out + getattr(err, "partial", ""), err.text, 1
    return out, "", 0


# ---- the device path's plain line (include/gtx.h) -------------------------------------------------------------------------------
_CANON = re.compile(r"(0|[1-9][0-9]{0,9})\Z")
_SCORE = re.compile(r"(0|-?[1-9][0-9]{0,17})\Z")


def is_plain(line):
    """3 to 6 tab-separated tokens, none empty or with a byte <= ' '; columns 2 and 3 canonical decimals of at most 10 digits below
    2^31 - 2 (column 2 + 1 too); column 5 a canonical long of at most 18 digits; column 6 exactly + or -"""
    tok = line.split("\t")
    if not 3 <= len(tok) <= 6:
        return False
    for t in tok:
        if t == "" or any(ord(c) <= 32 for c in t):
            return False
    for t in tok[1:3]:
        if not _CANON.match(t):
            return False
    if int(tok[1]) + 1 >= 2 ** 31 - 2 or int(tok[2]) >= 2 ** 31 - 2:
        return False
    if len(tok) >= 5 and not _SCORE.match(tok[4]):
        return False
    if len(tok) == 6 and tok[5] not in ("+", "-"):
        return False
    return True


def run_plain(op, text):
    """what the device prints for a block of plain lines: columns 1 and 4-6 copied, 2 and 3 rendered.  Independent of read_bed /
    render above: it is the claim of gtx.h that on plain lines the two agree"""
    out = ""
    for line in text.split("\n")[:-1]:
        assert is_plain(line), line
        tok = line.split("\t")
        r = {"chrom": tok[0], "strand": tok[5] if len(tok) == 6 else "+", "iv": [[int(tok[1]) + 1, int(tok[2])]], "thick": [0, 0]}
        if apply(op, r) and r["iv"]:
            out += "\t".join([tok[0], "%d" % (r["iv"][0][0] - 1), "%d" % r["iv"][0][1]] + tok[3:]) + "\n"
    return out
