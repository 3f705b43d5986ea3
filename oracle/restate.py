"""The reference's offset and bin rules restated in Python, and the region helpers of the join tests -- TEST INFRASTRUCTURE ONLY.

Imported by tests/; never by the product.  GetOffsetFrom (genomic_intervals.cpp:646-667), CalcOffsetsWithoutGaps (:6154-6205),
the bin index's order (:5619-5674) and the x / z / bin arithmetic of genomic_apps profile / heatmap (gtools/genomic_apps.cpp:560-605,
:826-880) are written here once for every test that checks them.
"""
import numpy as np

NAMES = ["chr1", "chr2", "chr3"]


# ---- the reference, restated ----

def offset_from(riv, minus, op, s, e):
    """GenomicInterval::GetOffsetFrom(GenomicRegion *) of [s, e] from the region with intervals riv and this strand"""
    back = op == "2" or (minus and op == "5p") or (not minus and op == "3p")
    a, b = riv[-1] if back else riv[0]
    ref = {"1": a, "2": b, "5p": b if minus else a, "3p": a if minus else b}[op]
    if (minus and op == "5p") or (not minus and op == "3p"):
        return ref - e, ref - s
    return s - ref, e - ref


def sorted_disjoint(iv):
    return all(iv[k][0] >= iv[k - 1][0] and iv[k][0] > iv[k - 1][1] for k in range(1, len(iv)))


def offsets_without_gaps(qiv, riv, minus, op):
    """CalcOffsetsWithoutGaps: the offsets of every query interval inside a reference interval, less the gaps before it from the
    point; [] for the warning case (intervals not sorted and disjoint)"""
    if not sorted_disjoint(qiv) or not sorted_disjoint(riv):
        return []
    gap = [0] * len(riv)
    if op == "1" or (not minus and op == "5p") or (minus and op == "3p"):
        for k in range(1, len(riv)):
            gap[k] = gap[k - 1] + riv[k][0] - riv[k - 1][1] - 1
    else:
        for k in range(len(riv) - 2, -1, -1):
            gap[k] = gap[k + 1] + riv[k + 1][0] - riv[k][1] - 1
    out = []
    for k, (rs, re_) in enumerate(riv):
        for qs, qe in qiv:
            if qs >= rs and qe <= re_:
                a, b = offset_from(riv, minus, op, qs, qe)
                out.append((a - gap[k], b - gap[k]))
    return out


def signal_bin(a, b, ref_len, bin_min, bin_max, n_bins):
    """the bin of offsets (a, b) in IEEE doubles, in the reference's order; n_bins is one past the reference's array (the pair is
    dropped), None when z lies outside [0, 1)"""
    x = float(a + b) / 2 / ref_len + bin_min
    z = (x - bin_min) / (bin_max - bin_min)
    return int(n_bins * z) if 0 <= z < 1 else None


def bin_keys(r, bits="17,20,23,26"):
    """the bin index's order as a key per region: (level, bin, -ordinal) ranked"""
    b = [int(x) for x in bits.split(",")] + [60]                               # the level after the last one given holds the rest
    s = np.maximum(r["s"], 1); e = r["e"]
    level = np.full(len(s), len(b), dtype=np.int64); bins = np.zeros(len(s), dtype=np.int64)
    for li in range(len(b) - 1, -1, -1):
        same = (s >> b[li]) == (e >> b[li])
        level = np.where(same, li, level); bins = np.where(same, s >> b[li], bins)
    order = np.lexsort((-np.arange(len(s)), bins, level))
    key = np.empty(len(s), dtype=np.int64); key[order] = np.arange(len(s))
    return key


def parse(line):
    """a BED line (3 to 12 columns) as GenomicRegionBED::Read takes it: 1-based inclusive intervals iv, envelope s / e"""
    t = line.split("\t")
    n = len(t)
    start = int(t[1]) + 1
    if n == 12:
        sizes = [int(x) for x in t[10].split(",") if x]; starts = [int(x) for x in t[11].split(",") if x]
        iv = [(start + b, start + b + a - 1) for a, b in zip(sizes, starts)]
    else:
        iv = [(start, int(t[2]))]
    strand = t[5] if n > 5 else "+"
    return dict(n=n, chrom=t[0], label=t[3] if n > 3 else "_", score=int(t[4]) if n > 4 else 0, strand=strand, minus=strand == "-",
                ts=int(t[6]) if n > 7 else 0, te=int(t[7]) if n > 7 else 0, rgb=t[8] if n > 8 else "", iv=iv, s=iv[0][0], e=iv[-1][1])


# ---- regions as a dict of arrays: chrom, strand (0 '+', 1 '-'), 1-based inclusive s / e, interval lists (first, blocks) ----

def regions(rng, n, span, lmin, lmax, n_chrom=3, sort="pos", multi=0.0, wide=0, block_max=60):
    """n random regions; a fraction `multi` has 2-4 intervals of 5 to block_max - 1 bases; `wide` regions span a third of the span
    or more.  sort: "pos" (chromosome, start), "strand" (chromosome, strand, start), anything else shuffled"""
    chrom = rng.integers(0, n_chrom, size=n)
    strand = rng.integers(0, 2, size=n)
    s = rng.integers(1, span, size=n)
    length = rng.integers(lmin, lmax + 1, size=n)
    if wide:
        at = rng.choice(n, wide, replace=False)
        length[at] = rng.integers(span // 3, span, size=wide)
    first, blocks = [0], []
    e = np.zeros(n, dtype=np.int64)
    for i in range(n):
        if rng.random() < multi:
            at, iv = int(s[i]), []
            for _ in range(int(rng.integers(2, 5))):
                sz = int(rng.integers(5, block_max)); iv.append((at, at + sz - 1)); at += sz + int(rng.integers(20, 400))
        else:
            iv = [(int(s[i]), int(s[i]) + int(length[i]) - 1)]
        e[i] = iv[-1][1]; blocks += iv; first.append(len(blocks))
    r = dict(chrom=chrom, strand=strand, s=s.astype(np.int64), e=e, first=np.array(first, dtype=np.int64),
             blocks=np.array(blocks, dtype=np.int64).reshape(-1, 2))
    if sort == "pos":
        return take(r, np.lexsort((r["s"], r["chrom"])))
    if sort == "strand":
        return take(r, np.lexsort((r["s"], r["strand"], r["chrom"])))
    return take(r, rng.permutation(n))


def take(r, order):
    cnt = np.diff(r["first"])[order]
    first = np.concatenate(([0], np.cumsum(cnt))).astype(np.int64)
    blocks = np.concatenate([r["blocks"][r["first"][i]:r["first"][i + 1]] for i in order]) if len(order) else r["blocks"][:0]
    out = {k: np.asarray(r[k])[order] for k in ("chrom", "strand", "s", "e")}
    out.update(first=first, blocks=blocks.reshape(-1, 2))
    return out


def concat(a, b):
    r = {k: np.concatenate((a[k], b[k])) for k in ("chrom", "strand", "s", "e")}
    r["blocks"] = np.concatenate((a["blocks"], b["blocks"]))
    r["first"] = np.concatenate((a["first"], a["first"][-1] + b["first"][1:]))
    return r


def write_bed(path, r, prefix, names=NAMES):
    with open(path, "w") as f:
        for i in range(len(r["s"])):
            b = r["blocks"][r["first"][i]:r["first"][i + 1]]
            cols = [names[r["chrom"][i]], str(r["s"][i] - 1), str(r["e"][i]), "%s%d" % (prefix, i), "0", "+-"[r["strand"][i]]]
            if len(b) > 1:
                cols += [str(r["s"][i] - 1), str(r["e"][i]), "0", str(len(b)), ",".join(str(int(x[1] - x[0] + 1)) for x in b) + ",",
                         ",".join(str(int(x[0] - r["s"][i])) for x in b) + ","]
            f.write("\t".join(cols) + "\n")


def triples(r, ignore_strand, n_known=len(NAMES)):
    """class = chromosome (x2 + strand unless -i); a chromosome the reference set lacks gets a class outside [0, n_classes)"""
    c = r["chrom"] * (1 if ignore_strand else 2) + (0 if ignore_strand else r["strand"])
    c = np.where(r["chrom"] >= n_known, 10_000, c)
    return np.stack([c, r["s"], r["e"]], axis=1).astype(np.int32)


def multi(r):
    return None if (np.diff(r["first"]) == 1).all() else (r["first"], r["blocks"].astype(np.int32))
