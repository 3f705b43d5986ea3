"""Inputs of the conversion's tests (test_convert_cli_cpu.py, test_gpu_convert.py, test_gpu_convert_cli.py): line makers for the
three formats, seeded files in which plain lines are mixed with lines only the host loop takes, and the operations they run with."""
import numpy as np

FMT_EXT = {"sam": "sam", "gff": "gff", "bed": "bed"}
OPS = {
    "sam": [{"to": "bed"}, {"to": "reg"}, {"to": "bed", "chr": True, "color": "255,0,0", "title": "reads", "position": "chr1:1-1000"}, {"to": "reg", "compact": True}],
    "gff": [{"to": "bed"}, {"to": "reg"}, {"to": "bed", "chr": True, "color": "7"}],
    "bed": [{"to": "reg"}, {"to": "reg", "compact": True}],
}


def sam_line(qname, flag, rname, pos, cigar, seq=None, tags=()):
    """an alignment whose SEQ and QUAL are as long as the CIGAR's fragment (M I S X), unless seq is given"""
    if seq is None:
        n, frag = "", 0
        for c in cigar:
            if c.isdigit():
                n += c
            else:
                frag += int(n) if c in "MISX=" else 0
                n = ""
        seq = ("ACGT" * (frag // 4 + 1))[:frag] or "*"
    qual = "I" * len(seq) if seq != "*" else "*"
    return "\t".join([qname, str(flag), rname, str(pos), "30", cigar, "*", "0", "0", seq, qual] + list(tags))


def gff_line(seqname, start, stop, strand, label=None, comment=None, feature="exon"):
    cols = [seqname, "src", feature, str(start), str(stop), ".", strand, "."]
    if label is not None:
        cols.append(label)
        if comment is not None:
            cols.append(comment)
    return "\t".join(cols)


def plain_sam(n, seed, read_len=100, chroms=("chr1", "chr2", "chrX")):
    """n reads of read_len bp with an NM tag, some 250 bytes a line"""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(1, 200_000_000, n))
    flags = rng.choice([0, 16, 83, 99, 147, 163], n)
    seq = "ACGT" * (read_len // 4) + "ACGT"[:read_len % 4]
    return [sam_line("read%d" % k, int(flags[k]), chroms[k * len(chroms) // n], int(pos[k]), "%dM" % read_len, seq, ("NM:i:0", "MD:Z:%d" % read_len)) for k in range(n)]


def plain_gff(n, seed):
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(1, 200_000_000, n))
    return [gff_line("chr%d" % (1 + k * 3 // n), int(pos[k]), int(pos[k]) + int(rng.integers(0, 3000)), "+-"[int(rng.integers(0, 2))],
                     'gene_id "G%d"; transcript_id "T%d"; exon_number %d;' % (k // 7, k // 3, k % 3 + 1)) for k in range(n)]


def plain_bed(n, seed):
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, 200_000_000, n))
    out = []
    for k in range(n):
        cols = ["chr%d" % (1 + k * 3 // n), str(int(pos[k])), str(int(pos[k]) + int(rng.integers(1, 500))), "r%d" % k, str(int(rng.integers(0, 1000))), "+-"[int(rng.integers(0, 2))]]
        out.append("\t".join(cols[:int(rng.integers(3, 7))]))
    return out


def seeded_lines(fmt, seed, n=3000):
    """a plain line first (the set's format is read off it), then plain lines mixed with lines that are not plain and no error"""
    rng = np.random.default_rng(seed)
    plain = {"sam": plain_sam, "gff": plain_gff, "bed": plain_bed}[fmt](n, seed + 1000)
    out = [plain[0]]
    for k in range(1, n):
        kind = int(rng.integers(0, 12))
        s = int(rng.integers(1, 2_000_000))
        strand = "+-"[int(rng.integers(0, 2))]
        if kind < 7:
            out.append(plain[k])
        elif fmt == "sam":
            flag = int(rng.choice([0, 16, 99, 147]))
            if kind == 7:
                out.append(sam_line("s%d" % k, flag, "chr1", s, "%dM%dN%dM" % (rng.integers(1, 60), rng.integers(1, 5000), rng.integers(1, 60))))
            elif kind == 8:
                out.append(sam_line("t%d" % k, flag, "chr2", s, "20M300N5M2I5M1000N30M", tags=("XS:A:+",)))
            elif kind == 9:
                out.append(sam_line("sign%d" % k, "+%d" % flag, "chr2", "+%d" % s, "36M"))
            elif kind == 10:
                out.append(sam_line("two words %d" % k, flag, "MT", " %d" % s, "36M"))
            else:
                out.append(sam_line("cr%d" % k, flag, "chrX", s, "50M", tags=("NM:i:1",) if k % 2 else ()) + "\r")
        elif fmt == "gff":
            ln = int(rng.integers(0, 900))
            if kind in (7, 8):
                out.append(gff_line("chr1", s, s + ln, ".", "ID=dot%d" % k))
            elif kind == 9:
                out.append(gff_line("chr2", "+%d" % s, s + ln, strand, "ID=sign%d" % k))
            elif kind == 10:
                out.append(gff_line("MT", s, s + ln, strand, " blank%d" % k, "note"))
            else:
                out.append(gff_line("chrX", s, s + ln, strand + "x", "ID=cr%d" % k) + "\r")
        else:
            cols = ["chr%d" % rng.integers(1, 4), str(s), str(s + int(rng.integers(0, 400))), "o%d" % k, str(int(rng.integers(-5, 1000))), strand]
            if kind == 7:
                out.append(" ".join(cols[:int(rng.integers(3, 7))]))
            elif kind == 8:
                out.append("\t".join(cols[:5] + [[".", "1", "-1"][int(rng.integers(0, 3))]]))
            elif kind == 9:
                out.append("\t".join(cols + [str(s + 5)]))
            elif kind == 10:
                out.append("\t".join([cols[0], "00%d" % s, "+%d" % (s + 9), cols[3], "007", "+"]))
            else:
                out.append("\t".join(cols + [str(s), str(s + 50), "0", "2", "10,20,", "0,%d," % (30 + k % 50)]))
    return "".join(l + "\n" for l in out)
