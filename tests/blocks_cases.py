"""Seeded generators of BED text for the block operations (genomic_blocks, gtx_blocks_text): plain lines of 3 to 6 columns, plain
12-column lines with a chosen number of blocks, and the odd lines -- lines the device does not take but every operation's host loop
prints without an error -- by kind.  blocks_restate.is_plain says which is which; the tests assert it."""
import random

CHROMS = ("chr1", "chr2", "chr10", "chrX", "MT", "scaffold_123456.1")
ODD_KINDS = ("cols7", "cols8", "cols9", "cols10", "cols11", "blanks", "dot_strand", "one_strand", "minus_one_strand", "leading_zero",
             "first_start", "last_stop", "count_short", "zero_size", "plus_number", "double_comma")


def label(rng, n=None):
    n = n or rng.randint(1, 12)
    return "".join(rng.choice("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_.:|") for _ in range(n))


def score(rng):
    return rng.choice(["0", "1", "1000", "-5", str(rng.randint(-10 ** 6, 10 ** 6)), "999999999999999999", "-999999999999999999"])


def plain_short(rng, cols=None, start=None, size=None):
    """a plain line of 3 to 6 columns (start > stop happens: nothing about the interval is checked)"""
    cols = cols or rng.randint(3, 6)
    a = rng.randint(0, 10 ** rng.randint(1, 8)) if start is None else start
    z = a + (rng.randint(1, 5000) if size is None else size)
    if start is None and size is None and rng.random() < 0.03:
        z = max(0, a - rng.randint(0, 3))
    return "\t".join([rng.choice(CHROMS), str(a), str(z), label(rng), score(rng), rng.choice("+-")][:cols])


def blocks_of(rng, n, max_size=300, max_gap=2000, touch=0.15):
    """sizes and relative starts of n sorted blocks; a block touches the one before it with probability `touch`"""
    sizes, starts, at = [], [], 0
    for k in range(n):
        if k:
            at += 0 if rng.random() < touch else rng.randint(1, max_gap)
        size = rng.randint(1, max_size)
        sizes.append(size)
        starts.append(at)
        at += size
    return sizes, starts


def bed12(chrom, a, name, sc, strand, thick, rgb, sizes, starts, comma=True, stop=None, count=None):
    end = "," if comma else ""
    return "\t".join([chrom, str(a), str(a + starts[-1] + sizes[-1] if stop is None else stop), name, sc, strand, str(thick[0]), str(thick[1]), rgb,
                      str(len(sizes) if count is None else count), ",".join(map(str, sizes)) + end, ",".join(map(str, starts)) + end])


def plain12(rng, n=None, comma=None, start=None, **kw):
    """a plain 12-column line of n blocks; the thick pair lies inside, across an edge of, or outside the line"""
    n = n or rng.choice((1, 1, 2, 2, 3, 3, 4, 5, 8, 13))
    sizes, starts = blocks_of(rng, n, **kw)
    a = rng.randint(0, 10 ** rng.randint(1, 8)) if start is None else start
    z = a + starts[-1] + sizes[-1]
    mode = rng.randint(0, 4)
    thick = [(a, z), (rng.randint(a, z), rng.randint(a, z)), (max(0, a - rng.randint(0, 50)), z + rng.randint(0, 50)), (z + 5, z + 9), (0, 0)][mode]
    return bed12(rng.choice(CHROMS), a, label(rng), score(rng), rng.choice("+-"), thick, rng.choice(("0", "255,0,0", "0,0,255")), sizes, starts,
                 comma=rng.random() < 0.5 if comma is None else comma)


def plain(rng):
    return plain12(rng) if rng.random() < 0.6 else plain_short(rng)


def odd(rng, kind=None):
    """a line that is not plain and that no operation's host loop stops at"""
    kind = kind or rng.choice(ODD_KINDS)
    a = rng.randint(0, 10 ** 6)
    sizes, starts = blocks_of(rng, rng.randint(2, 5), touch=0)
    z = a + starts[-1] + sizes[-1]
    full = bed12(rng.choice(CHROMS), a, label(rng), score(rng), rng.choice("+-"), (a, z), "0", sizes, starts).split("\t")
    if kind.startswith("cols"):
        return "\t".join(full[:int(kind[4:])])
    if kind == "blanks":
        return " ".join(plain_short(rng, rng.randint(3, 6)).split("\t"))
    if kind == "dot_strand":
        full[5] = "."
    elif kind == "one_strand":
        full[5] = "1"
    elif kind == "minus_one_strand":
        full[5] = "-1"
    elif kind == "leading_zero":
        if rng.random() < 0.5:
            full[rng.choice((1, 2))] = "0" + full[1]
            return "\t".join(full[:rng.randint(3, 6)])
        full[rng.choice((1, 2, 6, 7))] = "0" + full[1]
    elif kind == "first_start":
        starts = [s + 3 for s in starts]
        full[11] = ",".join(map(str, starts)) + ","
        full[2] = str(a + starts[-1] + sizes[-1])
    elif kind == "last_stop":
        full[2] = str(z + 7)
    elif kind == "count_short":
        full[9] = str(len(sizes) - 1)
    elif kind == "zero_size":
        sizes[0] = 0
        full[10] = ",".join(map(str, sizes))
    elif kind == "plus_number":
        full[1] = "+" + full[1]
        return "\t".join(full[:rng.randint(3, 6)])
    elif kind == "double_comma":
        full[10] += ","
    return "\t".join(full)


def text_of(lines):
    return "".join(x + "\n" for x in lines)


def mixed(seed, n, odd_every=0):
    """n seeded lines, plain but for an odd one every odd_every lines"""
    rng = random.Random(seed)
    return [odd(rng) if odd_every and k % odd_every == odd_every - 1 else plain(rng) for k in range(n)]


def ops():
    """the operations the seeded comparisons run: every kind, select with each flag and with both ends, strand with each word"""
    from blocks_restate import make_op
    return [make_op("split"), make_op("connect"), make_op("diff"), make_op("n"),
            make_op("select", first=True), make_op("select", last=True), make_op("select", p5=True), make_op("select", p3=True),
            make_op("select", first=True, last=True), make_op("select", p5=True, p3=True, first=True),
            make_op("strand"), make_op("strand", strand_op="-"), make_op("strand", strand_op="r")]


def op_id(op):
    return "-".join(x.lstrip("-") for x in __import__("blocks_restate").tool_args(op)).replace("+", "plus") or op["kind"]
