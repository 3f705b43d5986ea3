"""Restatement in Python of `genomic_regions bed` and `genomic_regions reg` (genomic_convert), from the reference's source: the
options gtools/genomic_regions.cpp:485-490 and :583-585, the hidden header :702, the calls :710 and :722;
GenomicRegionSet::RunConvertToBED gtools/genomic_intervals.cpp:3940-3948 over GenomicRegion::PrintBEDFormat :1256-1274 and
PrintChromosome :5968-5972; RunConvertToREG :4097-4103 over PrintREG :961-971, Print :843-849 and PrintInterval :344-347; with the
readers GenomicRegionSAM::Read :2771-2812 (strand :2870-2873, the CIGAR :2888-2920), GenomicRegionGFF::Read :3501-3517 and, from
regionops_restate, GenomicRegionBED::Read :2157-2182.  Beside it is_plain: the lines the device takes (include/gtx.h)."""
import re

import regionops_restate as rr
from regionops_restate import InputError, Tokens, atol, count_tokens

FORMATS = ("sam", "gff", "bed")


def line_error(n_line, msg):
    return InputError("\nError: Line %d: %s\n" % (n_line, msg))


def read_sam(line, n_line):
    """GenomicRegionSAM::Read :2771-2812: label, chrom, strand and iv = [[start, stop], ..], one interval per run between N operations"""
    nt = count_tokens(line, "\t")
    if nt < 11:
        raise line_error(n_line, "number of tokens should be at least 11 for SAM format!")
    t = Tokens(line)
    label = t.next("\t")
    flag = atol(t.next("\t"))
    rname = t.next("\t")
    pos = atol(t.next("\t"))
    t.next("\t")
    cigar = t.next("\t")
    t.next("\t"), t.next("\t"), t.next("\t")
    seq = t.next("\t")
    if cigar == "*":
        cigar = "%dM" % len(seq)                                      # :2791
    ops = []
    for m in re.finditer(r"(\d*)(.)", cigar):                         # TokenizeCIGAR :2888-2920
        if m.group(2) not in "MIDNSHP-X":
            raise line_error(n_line, "unknown CIGAR operation type '%s'!" % m.group(2))
        ops.append((atol(m.group(1)), m.group(2)))
    if seq != "*" and len(seq) != sum(n for n, c in ops if c in "MIS=X"):       # :2793-2800
        raise line_error(n_line, "length of aligned fragment does not match CIGAR string: \n  LABEL = %s\n  CIGAR = %s\n  length(SEQ) = %d\n" % (label, cigar, len(seq)))
    strand = "-" if flag & 0x10 else "+"                              # :2870-2873
    iv, start, ref = [], pos, 0
    for n, c in ops:                                                  # :2801-2810
        if c != "N":
            if c in "MD=X":
                ref += n
        else:
            iv.append([start, start + ref - 1])
            start += ref + n
            ref = 0
    if ref > 0:
        iv.append([start, start + ref - 1])
    if not iv:                                                        # (the reference reads I.front() of an empty region: an input error in this build)
        raise line_error(n_line, "SAM alignment without a reference interval (its CIGAR string has no M, D, X or N operation of positive length)!")
    return {"n_line": n_line, "label": label, "chrom": rname, "strand": strand, "iv": iv}


def read_gff(line, n_line):
    """GenomicRegionGFF::Read :3501-3517: one interval, columns 4 and 5 as written; the strand is the first byte of column 7"""
    nt = count_tokens(line, "\t")
    if nt < 8 or nt > 10:
        raise line_error(n_line, "wrong number of tokens for GFF format!")
    t = Tokens(line)
    chrom = t.next("\t")
    t.next("\t"), t.next("\t")
    start, stop = atol(t.next("\t")), atol(t.next("\t"))
    t.next("\t")
    strand = t.next("\t")[:1]
    t.next("\t")
    label = "_" if nt == 8 else t.next("\t")
    return {"n_line": n_line, "label": label, "chrom": chrom, "strand": strand, "iv": [[start, stop]]}


def read(line, n_line, fmt):
    if fmt == "sam":
        return read_sam(line, n_line)
    if fmt == "gff":
        return read_gff(line, n_line)
    return rr.read_bed(line, n_line)


def bed_format(r, color, convert):
    """PrintBEDFormat :1256-1274"""
    iv = r["iv"]
    for k in range(1, len(iv)):                                       # :1258 (one chromosome and strand per region here)
        if iv[k][0] < iv[k - 1][0] or iv[k][0] <= iv[k - 1][1]:
            raise line_error(r["n_line"], "region intervals must be compatible, sorted and non-overlapping for this operation!")
    chrom = "chr" + ("M" if r["chrom"] == "MT" else r["chrom"]) if convert else r["chrom"]     # :5968-5972
    out = "%s\t%d\t%d\t%s\t%d\t%s" % (chrom, iv[0][0] - 1, iv[-1][1], r["label"], 1000, r["strand"])          # :1261
    if color or len(iv) > 1:                                          # :1262
        out += "\t%d\t%d\t%s" % (iv[0][0] - 1, iv[-1][1], color or "0")
    if len(iv) > 1:                                                   # :1263-1272
        out += "\t%d\t" % len(iv) + ",".join("%d" % (e - s + 1) for s, e in iv) + "\t0"
        out += "".join(",%d" % (s - iv[0][0]) for s, _ in iv[1:])
    return out + "\n"


def reg_format(r, compact):
    """PrintREG :961-971"""
    iv = r["iv"]
    if compact:                                                       # :964-968
        return "%s\t%s %s %s %s\n" % (r["label"], r["chrom"], r["strand"], ",".join("%d" % s for s, _ in iv), ",".join("%d" % e for _, e in iv))
    return r["label"] + "\t" + " ".join("%s %s %d %d" % (r["chrom"], r["strand"], s, e) for s, e in iv) + "\n"     # :843-849, :344-347


def is_header(line, fmt):
    if fmt == "sam":
        return line.startswith("@")
    if fmt == "gff":
        return line.startswith("##")
    return rr.is_header(line)


def run(op, text, fmt):
    """(stdout, stderr, exit status) of op = {"to": "bed" | "reg", "title", "color", "position", "chr", "compact"} (all but "to"
    optional) on the text of a file of format fmt; only complete lines count (core.cpp:241-259)"""
    assert fmt in FORMATS and op["to"] in ("bed", "reg") and not (fmt == "bed" and op["to"] == "bed")
    lines = text.split("\n")[:-1]
    k = 0
    while k < len(lines) and is_header(lines[k], fmt):                # hidden (genomic_regions.cpp:702)
        k += 1
    if k == len(lines):                                               # :3942, :4099
        return "", "", 0
    out = ""
    try:
        regions = [read(lines[k], k + 1, fmt)]                        # (the set's constructor reads the first region: its error comes before anything is printed)
    except InputError as err:
        return "", err.text, 1
    if op["to"] == "bed":                                             # :3944-3945
        if op.get("position"):
            out += "browser position %s\n" % op["position"]
        if op.get("title"):
            out += "track name='%s' itemRgb=On visibility=1\n" % op["title"]
    for n in range(k, len(lines)):
        try:
            r = regions.pop() if regions else read(lines[n], n + 1, fmt)
            out += bed_format(r, op.get("color") or "", bool(op.get("chr"))) if op["to"] == "bed" else reg_format(r, bool(op.get("compact")))
        except InputError as err:
            return out, err.text, 1
    return out, "", 0


def tool_args(op):
    """the options of genomic_convert for op"""
    a = [op["to"]]
    if op["to"] == "reg":
        return a + (["-c"] if op.get("compact") else [])
    for o, k in (("-t", "title"), ("-c", "color"), ("-p", "position")):
        if op.get(k):
            a += [o, op[k]]
    return a + (["-chr"] if op.get("chr") else [])


# ---- the device path's plain line (include/gtx.h) -------------------------------------------------------------------------------
_NUM = re.compile(r"[0-9]{1,10}\Z")
_CIGAR = re.compile(r"([0-9]{1,9}[MIDSHPX-])+\Z")
_LIMIT = 2 ** 31 - 2


def _clean(tok):
    return tok != "" and not any(c in " \r\0" for c in tok)


def is_plain(line, fmt):
    """would the tokenizer (GTX_TEXT_SAM, GTX_TEXT_GFF) or, for BED, the rewrite's predicate take the line?"""
    if fmt == "bed":
        return rr.is_plain(line)
    tok = line.split("\t")
    if line.endswith("\r"):
        return False
    if fmt == "sam":
        if len(tok) < 11 or not all(_clean(t) for t in tok[:10]) or tok[10] == "" or tok[10][0] in " \r\0":
            return False
        if not _NUM.match(tok[1]) or not _NUM.match(tok[3]):
            return False
        cigar, seq = tok[5], tok[9]
        if cigar == "*":
            ref = len(seq)
        else:
            if not _CIGAR.match(cigar):
                return False
            ops = [(int(n), c) for n, c in re.findall(r"([0-9]+)(.)", cigar)]
            ref = sum(n for n, c in ops if c in "MDX")
            if seq != "*" and len(seq) != sum(n for n, c in ops if c in "MISX"):
                return False
        pos = int(tok[3])
        return ref > 0 and pos < _LIMIT and pos + ref - 1 < _LIMIT
    if not 8 <= len(tok) <= 10 or not all(_clean(t) for t in tok[:8]):
        return False
    if not _NUM.match(tok[3]) or not _NUM.match(tok[4]) or tok[6] not in ("+", "-"):
        return False
    if len(tok) >= 9 and (tok[8] == "" or ord(tok[8][0]) <= 32):
        return False
    if len(tok) == 10 and tok[9] == "":
        return False
    return int(tok[3]) < _LIMIT and int(tok[4]) < _LIMIT
