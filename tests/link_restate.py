"""`genomic_regions link` restated in Python -- TEST INFRASTRUCTURE ONLY: the yardstick of the link tests.

The loop is the reference's RunGlobalLink (gtools/genomic_intervals.cpp:4605-4644), written as it stands there:
  * the first region is the head r0 of a group, new_stop = r0.STOP (:4614-4615);
  * the following region comes through Next(sorted_by_strand, ...) (:3874-3882), which stops with
    "input regions are not sorted (sorted-by-strand = true|false)!" when it IsBefore (:396-401: chromosome by strcmp, strand only
    when sorted_by_strand, START) the region in front of it -- the previous region, not the head;
  * a region with other than one interval is "not a single-interval region!" (:4613, :4620), AFTER Next's order check of its line;
  * it joins when the head IsCompatibleWith it (:416-421: same chromosome, same strand unless ignore_strand = !sorted_by_strand)
    and START - new_stop <= max_difference (:4622); then new_stop = max(STOP, new_stop) (:4623);
  * otherwise the group prints through PrintModified (:909-913): label TAB chromosome SPACE strand SPACE START(head) SPACE new_stop,
    chromosome and strand the head's, and the region heads the next group.
Labels (:4616-4637): "" prints "_"; min / max / sum fold atof(LABEL) in double in input order and print through stringstream (%g);
any other string is a delimiter between the members' labels.  PrintError (:1001-1006) writes "\\nError: Line N: msg\\n" and exits 1;
stdout holds the groups closed before that.  Header lines are echoed (genomic_regions.cpp: hide_header = false).
BED parsing is oracle/restate.py's (1-based inclusive coordinates: BED start + 1).

link_packed is the same loop on packed (class, start, stop) triples with int64 values: what the C ABI's gtx_link is held to.
"""
import re

import numpy as np

from oracle import restate

_ATOF = re.compile(r"^[ \t\n\v\f\r]*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|inf(inity)?|nan)", re.I)


def atof(s):
    m = _ATOF.match(s)
    return float(m.group(0)) if m else 0.0


def is_header(line):
    return line.startswith("browser ") or line.startswith("track ")


def is_before(a, b, sorted_by_strand):
    """GenomicInterval::IsBefore on the front intervals (:396-401); chromosomes compare as strcmp does (bytes)"""
    ca, cb = a["chrom"].encode(), b["chrom"].encode()
    if ca != cb:
        return ca < cb
    if sorted_by_strand and a["strand"] != b["strand"]:
        return a["strand"] < b["strand"]
    return a["iv"][0][0] < b["iv"][0][0]


def link_lines(lines, sorted_by_strand=False, max_difference=0, label_func=""):
    """(stdout, stderr, exit code) of `genomic_regions link` on the lines of a BED file (no newlines)"""
    out = []
    at = 0
    while at < len(lines) and is_header(lines[at]):
        out.append(lines[at] + "\n")
        at += 1
    regs = [(k + 1, restate.parse(lines[k])) for k in range(at, len(lines)) if lines[k] != ""]
    is_func = label_func in ("min", "max", "sum")

    def fail(n_line, msg):
        return "".join(out), "\nError: Line %d: %s\n" % (n_line, msg), 1

    i = 0
    while i < len(regs):
        n0, r0 = regs[i]
        if len(r0["iv"]) != 1:
            return fail(n0, "not a single-interval region!")
        new_stop = r0["iv"][0][1]
        new_label = r0["label"] if label_func else "_"
        new_val = atof(r0["label"])
        i += 1
        while i < len(regs):
            n, r = regs[i]
            if is_before(r, regs[i - 1][1], sorted_by_strand):
                return fail(n, "input regions are not sorted (sorted-by-strand = %s)!" % ("true" if sorted_by_strand else "false"))
            if len(r["iv"]) != 1:
                return fail(n, "not a single-interval region!")
            compatible = r0["chrom"] == r["chrom"] and (not sorted_by_strand or r0["strand"] == r["strand"])
            if not (compatible and r["iv"][0][0] - new_stop <= max_difference):
                break
            new_stop = max(r["iv"][0][1], new_stop)
            if label_func:
                if not is_func:
                    new_label += label_func + r["label"]
                elif label_func == "min":
                    new_val = min(new_val, atof(r["label"]))
                elif label_func == "max":
                    new_val = max(new_val, atof(r["label"]))
                else:
                    new_val = new_val + atof(r["label"])
            i += 1
        if is_func:
            new_label = "%g" % new_val
        out.append("%s\t%s %s %d %d\n" % (new_label, r0["chrom"], r0["strand"], r0["iv"][0][0], new_stop))
    return "".join(out), "", 0


def link_packed(tri, max_difference=0, values=None, fold=None):
    """the loop on (class, start, stop) rows: (heads, counts, stops, folded or None, first_unsorted); fold: "sum" | "min" | "max"
    over int64 values (the sum wraps like two's complement).  Groups closed before the first unsorted row only."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    n = len(tri)
    c, s, e = tri[:, 0].tolist(), tri[:, 1].tolist(), tri[:, 2].tolist()
    v = None if values is None else [int(x) for x in values]
    heads, counts, stops, folded = [], [], [], []
    first_unsorted = -1
    i = 0
    while i < n and first_unsorted < 0:
        h, new_stop = i, e[i]
        acc = v[i] if fold else 0
        i += 1
        while i < n:
            if (c[i], s[i]) < (c[i - 1], s[i - 1]):
                first_unsorted = i
                break
            if not (c[i] == c[h] and s[i] - new_stop <= max_difference):
                break
            new_stop = max(e[i], new_stop)
            if fold == "sum":
                acc += v[i]
            elif fold == "min":
                acc = min(acc, v[i])
            elif fold == "max":
                acc = max(acc, v[i])
            i += 1
        if first_unsorted >= 0:
            break
        heads.append(h); counts.append(i - h); stops.append(new_stop)
        folded.append(((acc + 2 ** 63) % 2 ** 64) - 2 ** 63)
    return (np.array(heads, dtype=np.uint32), np.array(counts, dtype=np.uint32), np.array(stops, dtype=np.int32),
            np.array(folded, dtype=np.int64) if fold else None, first_unsorted)
