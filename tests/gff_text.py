"""GFF / GTF features for the tests: a seeded generator, and a restatement of the reference's reader (GenomicRegionGFF::Read,
gtools/genomic_intervals.cpp:3501-3517; detection :3713-3759) that turns every feature into the BED6 line of the same chromosome,
strand and interval -- the region the product must make of it.  A GTF attribute string holds blanks that the fourth column of a
BED line cannot carry past the oracle's tokenizer in every position, so the restatement labels line k `r<k>` (or keeps a numeric
label, for --max-label-value); labels_of() maps that name back to the ninth column."""
import numpy as np

from sam_text import _atol, count_tokens


def read_gff(line):
    """-> (chrom, strand byte, label, start, stop) of one feature line, or ValueError(message after 'Error: Line N: ').
    start and stop are columns 4 and 5 as written: 1-based, inclusive.  label is column 9, "_" for an 8-column line."""
    n = count_tokens(line)
    if n < 8 or n > 10:
        raise ValueError("wrong number of tokens for GFF format!")
    tok = [t.lstrip(" ") for t in line.split("\t")]
    return tok[0], tok[6][:1], (tok[8] if n > 8 else "_"), _atol(tok[3]), _atol(tok[4])


def looks_like_gff(line):
    """DetectFileFormat on the first data line: 8, 9 or 10 TAB tokens, the sixth without '+' or '-'"""
    n = count_tokens(line)
    if n < 8 or n > 10:
        return False
    sixth = line.split("\t")[5].lstrip(" ")
    return "+" not in sixth and "-" not in sixth


def to_bed(line, k, numeric_label=False):
    """the BED6 line of the same region; the strand byte as it stands ('.' is '+' to BED: right where the strand is ignored)"""
    chrom, strand, label, start, stop = read_gff(line)
    return "\t".join([chrom, str(start - 1), str(stop), str(_atol(label)) if numeric_label else "r%d" % k, "0", strand])


def gff_file_to_bed(text, numeric_label=False):
    """a whole GFF file -> BED text; its leading '##' lines become 'track' lines, so that line numbers stay the same"""
    out, top = [], True
    for k, l in enumerate(text.split("\n")[:-1]):
        if top and l.startswith("##"):
            out.append("track name=header")
            continue
        top = False
        out.append(to_bed(l, k, numeric_label))
    return "\n".join(out) + "\n"


def labels_of(text):
    """{"r<k>": column 9 of line k, or "_"} for the data lines of a GFF file"""
    out, top = {}, True
    for k, l in enumerate(text.split("\n")[:-1]):
        if top and l.startswith("##"):
            continue
        top = False
        out["r%d" % k] = read_gff(l)[2]
    return out


FEATURES = ("exon", "CDS", "gene", "transcript", "UTR")


def make_gff(rng, n, names, lo=1000, hi=2_000_000, length=(20, 3000), tokens=9, numeric_label=False, header=True, sort=True,
             strands="+-", extra_chrom=None):
    """n features, sorted by (seqname in strcmp order, start) when sort; -> GFF text.  tokens: 8, 9 or 10 columns, or a tuple to draw
    from per line; column 9 is a GTF attribute string (blanks, quotes, semicolons) unless numeric_label; strands: the bytes to draw
    column 7 from.  The score column is '.' or a plain decimal: never a '+' or '-' (which would make the file BED)."""
    c = rng.integers(0, len(names), n)
    start = rng.integers(lo, hi, n)
    if sort:
        order = np.lexsort((start, np.array([names[i] for i in c])))
        c, start = c[order], start[order]
    ln = rng.integers(length[0], length[1], n)
    st = rng.integers(0, len(strands), n)
    sc = rng.integers(0, 4, n)
    lab = rng.integers(0, 9, n)
    ft = rng.integers(0, len(FEATURES), n)
    ntok = np.full(n, tokens) if isinstance(tokens, int) else rng.choice(list(tokens), n)
    lines = ["##gff-version 2", "##source-version tests 1", "##date 2026-01-01"] if header else []
    for i in range(n):
        name = names[c[i]] if extra_chrom is None or i % 89 else extra_chrom
        score = "." if sc[i] else "%d.%d" % (lab[i], sc[i] + i % 7)
        tok = [name, "tests", FEATURES[ft[i]], str(start[i]), str(start[i] + ln[i]), score, strands[st[i]], ".012"[i % 4]]
        if ntok[i] > 8:
            tok.append(str(lab[i]) if numeric_label else 'gene_id "G%d.%d"; transcript_id "T%d"; gene_name "n %d";' % (i, lab[i], i, i % 13))
        if ntok[i] > 9:
            tok.append("a comment, line %d" % i)
        lines.append("\t".join(tok))
    return "\n".join(lines) + "\n"
