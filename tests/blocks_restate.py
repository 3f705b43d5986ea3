"""Restatement in Python of `genomic_regions split | connect | select | diff | n | strand` on BED input (genomic_blocks), from the
reference's source (file:line of gtools/genomic_intervals.cpp unless said otherwise): the options gtools/genomic_regions.cpp:509-514,
:551-553, :600-605, :617-623, the header shown :702-704, the calls :715-733; the drivers' loops :3999-4017, :4071-4078, :4121-4127,
:4187-4193, :4350-4358; GenomicRegionBED::RunSplit :2502-2505 over PrintModified :2310-2314; GenomicRegion::Connect :1319-1339, Select
:1493-1521 (Sort is a no-op for BED, :2493-2496), Diff :1345-1361 with IsCompatibleSortedAndNonoverlapping :1153-1161 and PrintError
:1001-1006, RunSize :1451-1454 over GetSize :1047-1055 and :488-491, ModifyStrand :1607-1620; and, from regionops_restate, the reader
GenomicRegionBED::Read, UpdateThick :2326-2333 and Print :2188-2218.  Two conventions of this build where the reference prints an
unset member: a 3-column line has the label "_", a line of fewer than 5 tokens the score 0.  Beside it is_plain, the lines the
device takes (include/gtx.h, gtx_blocks_text), and run_plain, a second rendering of those lines from their columns as text."""
import re

import regionops_restate as rr
from regionops_restate import InputError, read_bed, render, update_thick

KINDS = ("split", "connect", "select", "diff", "n", "strand")
SELECT_FLAGS = ("first", "last", "5p", "3p")
MAX_BLOCKS = 1024
LIMIT = 2 ** 31 - 2


def make_op(kind, first=False, last=False, p5=False, p3=False, strand_op="+", by_chrstrand=False):
    assert kind in KINDS
    return {"kind": kind, "first": first, "last": last, "5p": p5, "3p": p3, "op": strand_op, "by_chrstrand": by_chrstrand}


def norm_op(d):
    """an operation as the manifest writes it (the keys that are set) with every key"""
    return make_op(d["kind"], bool(d.get("first")), bool(d.get("last")), bool(d.get("5p")), bool(d.get("3p")), d.get("op", "+"), bool(d.get("by_chrstrand")))


def select_ends(op, strand):
    """:1497-1499: is the first, is the last interval wanted?"""
    pos_first = op["first"] or (op["5p"] and strand == "+") or (op["3p"] and strand == "-")
    pos_last = op["last"] or (op["5p"] and strand == "-") or (op["3p"] and strand == "+")
    return pos_first, pos_last


def apply(op, r):
    """what the operation prints for the region r of read_bed, which it changes; InputError as the reference raises it"""
    kind, iv = op["kind"], r["iv"]
    if kind == "split":                                               # :2502-2505, :2310-2314
        return "".join("%s\t%d\t%d\t%s\t%d\t%s\n" % (r["chrom"], s - 1, e, r["label"], r["score"], r["strand"]) for s, e in iv)
    if kind == "n":                                                   # :1451-1454
        return "%s\t%d\n" % (r["label"], sum(0 if s > e else e - s + 1 for s, e in iv))
    if kind == "connect":                                             # :1319-1339
        if len(iv) > 1:
            r["iv"] = [[min(s for s, _ in iv), max(e for _, e in iv)]]
        update_thick(r)
    elif kind == "select":                                            # :1493-1521
        pos_first, pos_last = select_ends(op, r["strand"])
        if not pos_first and not pos_last:
            r["iv"] = []
        elif len(iv) == 1:
            pass
        elif pos_first and pos_last:
            if len(iv) > 2:
                r["iv"] = [iv[0], iv[-1]]
        elif pos_first:
            r["iv"] = [iv[0]]
        else:
            r["iv"] = [iv[-1]]
        update_thick(r)
    elif kind == "diff":                                              # :1345-1361
        if len(iv) == 1:
            r["iv"] = []
        else:
            for k in range(1, len(iv)):                               # :1153-1161 (one chromosome and strand per BED region)
                if iv[k][0] < iv[k - 1][0] or iv[k][0] <= iv[k - 1][1]:
                    raise InputError("\nError: Line %d: region intervals must be compatible, sorted and non-overlapping for this operation!\n" % r["n_line"])
            r["iv"] = [[iv[k - 1][1] + 1, iv[k][0] - 1] for k in range(1, len(iv)) if iv[k][0] - 1 >= iv[k - 1][1] + 1]
        update_thick(r)
    else:                                                             # :1607-1620: another word changes nothing
        w = op["op"]
        if w == "r":
            r["strand"] = {"+": "-", "-": "+"}.get(r["strand"], r["strand"])
        elif w in ("+", "-"):
            r["strand"] = w
    return render(r)


def run(op, text):
    """(stdout, stderr, exit status) of the operation on the text of a BED file; only complete lines count (core.cpp:241-259)"""
    lines = text.split("\n")[:-1]
    out = ""
    k = 0
    while k < len(lines) and rr.is_header(lines[k]):                  # :3713-3720, hide_header = false (genomic_regions.cpp:702-704)
        out += lines[k] + "\n"
        k += 1
    for n in range(k, len(lines)):
        try:
            out += apply(op, read_bed(lines[n], n + 1))
        except InputError as err:
            return out + getattr(err, "partial", ""), err.text, 1
    return out, "", 0


def tool_args(op):
    """the options of genomic_blocks for op"""
    a = [op["kind"]]
    if op["kind"] == "split" and op["by_chrstrand"]:
        a += ["--by-chrstrand"]
    if op["kind"] == "select":
        a += ["-" + f for f in SELECT_FLAGS if op[f]]
    if op["kind"] == "strand" and op["op"] != "+":
        a += ["-op", op["op"]]
    return a


# ---- the device path's plain line (include/gtx.h) -------------------------------------------------------------------------------
_CANON = re.compile(r"(0|[1-9][0-9]{0,9})\Z")
_SCORE = re.compile(r"(0|-?[1-9][0-9]{0,17})\Z")


def _list(tok, n):
    """the n canonical decimals of a list with single commas and at most one trailing comma, or None"""
    if tok.endswith(","):
        tok = tok[:-1]
    items = tok.split(",")
    if len(items) != n or not all(_CANON.match(x) for x in items):
        return None
    return [int(x) for x in items]


def is_plain(line):
    """(a) 3 to 6 columns: regionops_restate.is_plain.  (b) exactly 12 tab-separated tokens, as include/gtx.h lists the conditions;
    the first block starts at 0 and the last ends at column 3 (a line that does not say so is left to the host loop)"""
    tok = line.split("\t")
    if len(tok) <= 6:
        return rr.is_plain(line)
    if len(tok) != 12 or any(t == "" or any(ord(c) <= 32 for c in t) for t in tok):
        return False
    if not all(_CANON.match(tok[k]) for k in (1, 2, 6, 7, 9)) or not _SCORE.match(tok[4]) or tok[5] not in ("+", "-"):
        return False
    s0, e, n = int(tok[1]), int(tok[2]), int(tok[9])
    if s0 + 1 >= LIMIT or e >= LIMIT or int(tok[6]) >= LIMIT or int(tok[7]) >= LIMIT or not 1 <= n <= MAX_BLOCKS:
        return False
    sizes, starts = _list(tok[10], n), _list(tok[11], n)
    if sizes is None or starts is None or min(sizes) < 1 or starts[0] != 0:
        return False
    for k in range(1, n):
        if starts[k] < starts[k - 1] + sizes[k - 1]:
            return False
    return s0 + starts[-1] + sizes[-1] == e and all(s0 + a + z < LIMIT for a, z in zip(starts, sizes))


def run_plain(op, text):
    """what the device prints for a block of plain lines, from the columns as text and 0-based block edges: independent of
    read_bed / render / apply above.  It is the claim of gtx.h that on plain lines the two agree"""
    out = []
    kind = op["kind"]
    for line in text.split("\n")[:-1]:
        assert is_plain(line), line
        t = line.split("\t")
        a, z = int(t[1]), int(t[2])
        strand = t[5] if len(t) >= 6 else "+"
        label = t[3] if len(t) >= 4 else "_"
        score = t[4] if len(t) >= 5 else "0"
        if len(t) == 12:
            n = int(t[9])
            sizes = [int(x) for x in t[10].rstrip(",").split(",")]
            starts = [int(x) for x in t[11].rstrip(",").split(",")]
            edges = [(a + starts[k], a + starts[k] + sizes[k]) for k in range(n)]          # (START-1, STOP] of every block
        else:
            edges = [(a, z)]

        def bed12(kept):
            lo, hi = kept[0][0], kept[-1][1]
            t0, t1 = max(int(t[6]), lo), min(int(t[7]), hi)
            if t1 <= t0:
                t0 = t1 = lo
            return "\t".join([t[0], str(lo), str(hi), t[3], t[4], strand, str(t0), str(t1), t[8], str(len(kept)),
                              ",".join(str(y - x) for x, y in kept), ",".join(str(x - lo) for x, _ in kept)]) + "\n"
        if kind == "split":
            out += ["\t".join([t[0], str(x), str(y), label, score, strand]) + "\n" for x, y in edges]
        elif kind == "n":
            out.append("%s\t%d\n" % (label, sum(max(0, y - x) for x, y in edges)))
        elif kind == "strand":
            new = {"+": "+", "-": "-", "r": "-" if strand == "+" else "+"}[op["op"]]
            u = list(t)
            if len(u) >= 6:
                u[5] = new
            if len(u) == 12:
                u[10], u[11] = u[10].rstrip(","), u[11].rstrip(",")
            out.append("\t".join(u) + "\n")
        elif kind == "connect":
            out.append(line + "\n" if len(t) < 12 else bed12([(a, z)]))
        elif kind == "select":
            first, last = select_ends(op, strand)
            if not first and not last:
                continue
            if len(t) < 12:
                out.append(line + "\n")
            elif first and last:
                out.append(bed12(edges if len(edges) <= 2 else [edges[0], edges[-1]]))
            else:
                out.append(bed12([edges[0] if first else edges[-1]]))
        else:
            gaps = [(edges[k - 1][1], edges[k][0]) for k in range(1, len(edges)) if edges[k][0] > edges[k - 1][1]]
            if gaps:
                out.append(bed12(gaps))
    return "".join(out)
