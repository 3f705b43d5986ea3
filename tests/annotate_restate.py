"""`genomic_overlaps annotate` restated in Python -- TEST INFRASTRUCTURE ONLY.

Two parts, each written from the reference's text and copied from none of it:
  * upstream_set: CreateGenomicRegionSetAnnotator (gtools/genomic_intervals.cpp:6218-6297) -- the upstream region of every gene
    (:6231-6241) and, when upstream_min < upstream_max, the trimming of every one against the untrimmed set in the order its own
    bin index hands the overlaps out (:6250-6294; GenomicRegionSetIndex::NextMatch :5489-5524, GetOverlap :5530-5555);
  * annotate: the loop of gtools/genomic_overlaps.cpp:310-353 and PrintAnnotations (:268-290) -- per test region its gene pairs
    (5p), then its upstream pairs (3p), each in that set's index order.
GetOffsetFrom and the bin order come from oracle/restate.py.  Regions are dicts: label, chrom, strand ('+' / '-'), s, e (1-based,
inclusive), line (1-based line in their file), n_iv (number of intervals).
"""
import numpy as np

from oracle.restate import bin_keys, offset_from, parse

HEADER = "TEST-LABEL\tTEST-LOCUS\tTEST-LOCUS-SIZE\tREF-LABEL\tREF-LOCUS\tREF-LOCUS-SIZE\tOFFSET\tNORMALIZED-OFFSET\n"
MULTI_REF = "single-interval reference regions are required for this operation!"
MULTI_TEST = "single-interval test regions are required for this operation!"
INDEX_BAD = "index regions should be compatible, sorted and non-overlapping!"
BAD_OP = "Error [PrintAnnotations]: invalid value for query operation!\n"
RANGE = "upstream region does not fit the packed 32-bit representation of the MI355X path!"
PACKED_MAX = 2 ** 31 - 2                                                        # coordinates of the MI355X path lie below it


class InputError(Exception):
    def __init__(self, line, msg):
        Exception.__init__(self, msg)
        self.line, self.msg = line, msg

    def stderr(self):
        return "\nError: Line %d: %s\n" % (self.line, self.msg)


def regions_of(lines):
    out = []
    for n, l in enumerate(lines):
        p = parse(l.replace(" ", "\t") if "\t" not in l else l)
        out.append(dict(label=p["label"], chrom=p["chrom"], strand=p["strand"], s=p["s"], e=p["e"], line=n + 1, n_iv=len(p["iv"]), iv=p["iv"]))
    return out


class Index:
    """the bin index over a list of regions: per region its key -- the rank of (level, bin, -ordinal), the order the index hands
    overlaps out in -- and the columns the overlap test reads; regions with start > stop or stop <= 0 are not in it (:5421)"""

    def __init__(self, regs, bits="17,20,23,26"):
        self.s = np.array([x["s"] for x in regs], dtype=np.int64)
        self.e = np.array([x["e"] for x in regs], dtype=np.int64)
        self.key = bin_keys(dict(s=self.s, e=self.e), bits) if len(regs) else np.zeros(0, dtype=np.int64)
        names = sorted({x["chrom"] for x in regs})
        self.code = {c: n for n, c in enumerate(names)}
        self.chrom = np.array([self.code[x["chrom"]] for x in regs], dtype=np.int64)
        self.minus = np.array([x["strand"] == "-" for x in regs], dtype=bool)
        self.valid = ~((self.s > self.e) | (self.e <= 0))


def index_order(regs, bits="17,20,23,26"):
    return Index(regs, bits)


def overlaps_in_order(regs, ix, chrom, strand, s, e, ignore_strand):
    """GetOverlap / NextOverlap under match_gaps = true: ordinals of the indexed regions the interval meets, in index order; an
    interval with stop <= 0 or start > stop meets nothing (:5500-5501)"""
    if e <= 0 or s > e or chrom not in ix.code:
        return []
    s = max(s, 1)
    m = ix.valid & (ix.chrom == ix.code[chrom]) & (ix.s <= e) & (ix.e >= s)
    if not ignore_strand:
        m &= ix.minus == (strand == "-")
    hit = np.flatnonzero(m)
    return hit[np.argsort(ix.key[hit])].tolist()


def upstream_set(genes, bounds, ignore_strand, upstream_max, upstream_min, bits="17,20,23,26"):
    """bounds: dict chromosome -> length, or None; a chromosome it does not name reads as 0 (and is inserted, as operator[] does)"""
    up = []
    for g in genes:
        if g["n_iv"] != 1:
            raise InputError(g["line"], MULTI_REF)
        if g["strand"] == "+":
            s, e = max(g["s"] - upstream_max, 1), max(g["s"] - 1, 1)
        else:
            s, e = g["e"] + 1, g["e"] + upstream_max
        if bounds is not None:
            e = min(e, bounds.setdefault(g["chrom"], 0))
        if s >= PACKED_MAX or e >= PACKED_MAX:
            raise InputError(g["line"], RANGE)
        up.append(dict(label="upstream:" + g["label"], chrom=g["chrom"], strand=g["strand"], s=s, e=e, line=len(up) + 1, n_iv=1, gene=g))
    if not upstream_min < upstream_max:
        return up
    key = index_order(up, bits)
    kept = []
    for k, u in enumerate(up):
        s, e = u["s"], u["e"]
        for j in overlaps_in_order(up, key, u["chrom"], u["strand"], u["s"], u["e"], ignore_strand):
            o = up[j]
            if j == k or o["strand"] != u["strand"]:
                continue
            if u["strand"] == "+":
                if u["e"] > o["e"]:
                    s = max(s, o["e"] + 1)
                    if upstream_min > 0 and e - s + 1 < upstream_min:
                        s = max(1, e - upstream_min + 1)
            elif o["s"] > u["s"]:
                e = min(e, o["s"] - 1)
                if upstream_min > 0 and e - s + 1 < upstream_min:
                    e = s + upstream_min - 1
                    if bounds is not None:
                        e = min(e, bounds.setdefault(o["chrom"], 0))
            if s > e:
                break
        if s <= e:
            if s >= PACKED_MAX or e >= PACKED_MAX:
                raise InputError(u["gene"]["line"], RANGE)
            kept.append(dict(u, s=s, e=e, line=len(kept) + 1))
    return kept


def reg_lines(regs):
    """the set as `genomic_regions annotator` prints it (gtools/genomic_intervals.cpp:4488): REG lines"""
    return "".join("%s\t%s %s %d %d\n" % (r["label"], r["chrom"], r["strand"], r["s"], r["e"]) for r in regs)


def pair_value(ref, three_prime, s, e, center):
    """PrintAnnotations :271-274: (printed?, the offset as the reference's double, the integer the device keeps)"""
    so, eo = offset_from([(ref["s"], ref["e"])], ref["strand"] == "-", "3p" if three_prime else "5p", s, e)
    if center:
        return so + eo >= 0, (so + eo) / 2, so + eo
    return True, float(so), so


def c_long(x):
    return int(x)                                                               # (long int) of a double: towards zero


def line_of(t, ref, three_prime, offset, flag, proximal):
    tag = ""
    if flag:
        tag = ("distal" if offset >= proximal else "proximal") + ":" if three_prime else ("distal" if offset > proximal else "proximal") + ":downstream:"
    size = ref["e"] - ref["s"] + 1
    return "%s\t%s %s %d %d\t%d\t%s%s\t%s %s %d %d\t%d\t%d\t%s\n" % (
        t["label"], t["chrom"], t["strand"], t["s"], t["e"], t["e"] - t["s"] + 1, tag, ref["label"], ref["chrom"], ref["strand"], ref["s"], ref["e"],
        size, c_long(offset), "%f" % (offset / size))


def compatible(r):
    iv = r["iv"]
    return all(iv[k][0] >= iv[k - 1][0] for k in range(1, len(iv))) and all(iv[k][0] > iv[k - 1][1] for k in range(1, len(iv)))


def annotate(gene_lines, test_lines, query_op="center", upstream_max=10000, upstream_min=10000, flag=False, proximal=1000, header=False,
             ignore_strand=False, bits="17,20,23,26", pairs=None):
    """(stdout, stderr, exit code) of `genomic_overlaps annotate` on BED lines.  pairs: None, or a function (set number 0 / 1, its
    regions) -> per test line (0-based) the ordinals it meets in index order, from another implementation of the bin index."""
    genes, tests = regions_of(gene_lines), regions_of(test_lines)
    out = ""
    try:
        for g in genes:
            if not compatible(g):
                raise InputError(g["line"], INDEX_BAD)
        up = upstream_set(genes, None, ignore_strand, upstream_max, upstream_min, bits) if upstream_max > 0 else None
        if header:
            out += HEADER
        sets = [genes] + ([up] if up is not None else [])
        keys = [index_order(s, bits) for s in sets]
        given = [pairs(n, s) if pairs else None for n, s in enumerate(sets)]
        for i, t in enumerate(tests):
            if t["n_iv"] != 1:
                raise InputError(t["line"], MULTI_TEST)
            for n, regs in enumerate(sets):
                hits = given[n][i] if given[n] is not None else overlaps_in_order(regs, keys[n], t["chrom"], t["strand"], t["s"], t["e"], ignore_strand)
                for k in hits:
                    ref = regs[k]
                    if ref["n_iv"] != 1:
                        raise InputError(ref["line"], MULTI_REF)
                    if query_op not in ("center", "overlap"):
                        return out, BAD_OP, 1
                    ok, offset, _ = pair_value(ref, n == 1, t["s"], t["e"], query_op == "center")
                    if ok:
                        out += line_of(t, ref, n == 1, offset, flag, proximal)
    except InputError as err:
        return out, err.stderr(), 1
    return out, "", 0
