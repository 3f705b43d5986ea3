"""SAM alignments for the tests: a seeded generator, and a restatement of the reference's reader (GenomicRegionSAM::Read,
gtools/genomic_intervals.cpp:2771-2812) that turns every alignment into the BED6 line (one interval) or BED12 line (a spliced read)
of the same chromosome, strand, label and intervals -- the region the product must make of it."""
import numpy as np

SAM_OPS = "MIDNSHP-X"          # what the reference's tokenizer accepts ('=' is refused)
REF_OPS = "MD=X"               # reference length
FRAG_OPS = "MIS=X"             # fragment length (strlen(SEQ))


def _atol(s):
    s = s.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in "+-" and s[:1]:
        sign, i = (-1 if s[0] == "-" else 1), 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    return sign * int(s[i:j]) if j > i else 0


def count_tokens(s, delim="\t"):
    """CountTokens (gtools/core.cpp:577-591): blanks in front of a token are skipped, a trailing delimiter adds no token"""
    k, n = 0, 0
    while k < len(s) and s[k] == " ":
        k += 1
    while k < len(s):
        while k < len(s) and s[k] != delim:
            k += 1
        if k < len(s):
            k += 1
        n += 1
        while k < len(s) and s[k] == " ":
            k += 1
    return n


def _in(op, ops):
    """strchr(ops, op) != NULL: the terminator, op "\\0", is found in every set"""
    return op == "\0" or op in ops


def cigar_ops(cigar):
    """(length, op) pairs as GetNextTokenOfCIGAR reads them; raises ValueError with the reference's message.  Digits at the end (no
    operation behind them) are an operation of type "\\0", and the CIGAR ends there (the reference reads on past
    the string)."""
    ops, p = [], 0
    while p < len(cigar):
        d = p
        while p < len(cigar) and cigar[p].isdigit():
            p += 1
        if p == len(cigar):
            ops.append((int(cigar[d:p]), "\0"))
            break
        op = cigar[p]
        if op not in SAM_OPS:
            raise ValueError("unknown CIGAR operation type '%s'!" % op)
        ops.append((int(cigar[d:p]) if p > d else 0, op))
        p += 1
    return ops


def read_sam(line):
    """-> (chrom, strand, label, [(start, stop), ...]) of one alignment line, or ValueError(message after 'Error: Line N: ')."""
    if count_tokens(line) < 11:
        raise ValueError("number of tokens should be at least 11 for SAM format!")
    tok = [t.lstrip(" ") for t in line.split("\t")]
    qname, flag, rname, pos, cigar, seq = tok[0], _atol(tok[1]), tok[2], _atol(tok[3]), tok[5], tok[9]
    strand = "-" if (flag & 0x10) else "+"
    if cigar == "*":
        cigar = "%dM" % len(seq)
    ops = cigar_ops(cigar)
    if seq != "*" and len(seq) != sum(n for n, o in ops if _in(o, FRAG_OPS)):
        raise ValueError("length of aligned fragment does not match CIGAR string: \n  LABEL = %s\n  CIGAR = %s\n  length(SEQ) = %d\n" % (qname, cigar, len(seq)))
    iv, start, ref = [], pos, 0
    for n, o in ops:
        if o != "N":
            if _in(o, REF_OPS):
                ref += n
        else:
            iv.append((start, start + ref - 1))
            start, ref = start + ref + n, 0
    if ref > 0:
        iv.append((start, start + ref - 1))
    if not iv:
        raise ValueError("SAM alignment without a reference interval (its CIGAR string has no M, D, X or N operation of positive length)!")
    return rname, strand, qname, iv


def to_bed(line):
    """the BED6 / BED12 line of the same region"""
    chrom, strand, label, iv = read_sam(line)
    s0, e0 = iv[0][0] - 1, iv[-1][1]
    if len(iv) == 1:
        return "\t".join([chrom, str(s0), str(e0), label, "0", strand])
    sizes = ",".join(str(e - s + 1) for s, e in iv) + ","
    starts = ",".join(str(s - iv[0][0]) for s, e in iv) + ","
    return "\t".join([chrom, str(s0), str(e0), label, "0", strand, str(s0), str(e0), "0", str(len(iv)), sizes, starts])


def sam_file_to_bed(text):
    """a whole SAM file -> BED text; its '@' header lines become 'track' lines, so that line numbers stay the same"""
    out, top = [], True
    for l in text.split("\n")[:-1]:
        if top and l.startswith("@"):
            out.append("track name=header")
            continue
        top = False
        out.append(to_bed(l.rstrip("\r")))
    return "\n".join(out) + "\n"


def random_cigar(rng, spliced, read_len, dash=True):
    """-> (cigar, fragment length): clips, indels, padding, '-' and X, an N when spliced; at least one M"""
    parts, frag = [], 0
    if rng.random() < 0.2:
        k = int(rng.integers(1, 6)); parts.append("%dS" % k); frag += k
    if rng.random() < 0.1:
        parts.insert(0, "%dH" % int(rng.integers(1, 6)))
    left = read_len
    nseg = int(rng.integers(2, 4)) if spliced else 1
    for s in range(nseg):
        m = max(1, left // (nseg - s) - int(rng.integers(0, 3)))
        left -= m
        parts.append("%dM" % m); frag += m
        if rng.random() < 0.15:
            k = int(rng.integers(1, 4)); parts.append("%dI" % k); frag += k
        if rng.random() < 0.15:
            parts.append("%dD" % int(rng.integers(1, 4)))
        if rng.random() < 0.05:
            parts.append("1P")
        if dash and rng.random() < 0.05:
            parts.append("2-")
        if rng.random() < 0.1:
            parts.append("%dX" % 2); frag += 2
        if s + 1 < nseg:
            parts.append("%dN" % int(rng.integers(0, 3000)))
    return "".join(parts), frag


def make_sam(rng, n, names, lo=1000, hi=2_000_000, read_len=60, spliced=0.0, numeric_qname=False, header=True, sort=True,
             star_cigar=0.02, star_seq=0.05, chrom_weights=None, extra_chrom=None):
    """n alignments, sorted by (RNAME in strcmp order, POS) when sort; -> SAM text"""
    c = rng.integers(0, len(names), n) if chrom_weights is None else rng.choice(len(names), n, p=chrom_weights)
    pos = rng.integers(lo, hi, n)
    if sort:
        order = np.lexsort((pos, np.array([names[i] for i in c])))
        c, pos = c[order], pos[order]
    lines = ["@HD\tVN:1.6\tSO:coordinate"] + ["@SQ\tSN:%s\tLN:%d" % (nm, hi + 10000) for nm in names] if header else []
    for i in range(n):
        rl = int(rng.integers(read_len // 2, read_len + 1))
        flag = int(rng.choice([0, 16, 256, 272, 1, 17]))
        if rng.random() < star_cigar:
            cigar, frag = "*", rl
        else:
            cigar, frag = random_cigar(rng, rng.random() < spliced, rl, dash=i > 0)     # (a '-' in the first line's 6th column: BED)
        seq = "*" if rng.random() < star_seq else "".join(rng.choice(list("ACGTN"), frag))
        qual = "*" if seq == "*" else "I" * len(seq)
        qname = str(int(rng.integers(0, 9))) if numeric_qname else "q%d" % i
        rname = names[c[i]] if extra_chrom is None or i % 89 else extra_chrom
        tags = ["", "\tNM:i:0", "\tNM:i:0\tAS:i:%d" % frag][int(rng.choice(3, p=[0.3, 0.3, 0.4]))]     # 11, 12 or 13 columns
        lines.append("%s\t%d\t%s\t%d\t%d\t%s\t=\t%d\t0\t%s\t%s%s" % (qname, flag, rname, pos[i], int(rng.integers(0, 61)), cigar,
                                                                   pos[i] + 200, seq, qual, tags))
    return "\n".join(lines) + "\n"
