"""Restatement in Python of `genomic_regions win` on BED input, from the reference's source: the options gtools/genomic_regions.cpp
:647-651, the call :734, GenomicRegionSet::RunSlidingWindows gtools/genomic_intervals.cpp:4449-4455 over
GenomicRegionBED::PrintWindows :2520-2532, with the reader (:2157-2182), the header echo and the error of a line taken from
regionops_restate.  Beside it, as separate functions, the closed forms the device path plans with (csrc/gtx_windows.h): the number
of windows of a line, the number of full-size ones, and the bytes of a line's first k windows from digit counts of two arithmetic
progressions."""
import regionops_restate as rr
from regionops_restate import InputError, is_plain, read_bed   # noqa: F401  (is_plain: the device's notion of a plain line)


def windows_of(r, step, size, small):
    """PrintWindows :2520-2532 of a region read_bed returned: the printed text.  step >= 1 (the loop does not advance otherwise)"""
    if len(r["iv"]) != 1:
        raise InputError("\nError: Line %d: this operation requires single-interval regions!\n\n" % r["n_line"])     # :2522
    start, stop = r["iv"][0]
    out = []
    z = start
    while z <= stop:                                                  # :2523
        if not small and z + size - 1 > stop:                         # :2524
            break
        line = "%s\t%d\t%d" % (r["chrom"], z - 1, min(z + size - 1, stop))        # :2525
        if r["n_tokens"] >= 4:                                        # :2526-2529
            line += "\t" + r["label"]
            if r["n_tokens"] >= 6:
                line += "\t%d\t%s" % (r["score"], r["strand"])
        out.append(line + "\n")
        z += step
    return "".join(out)


def run(op, text):
    """(stdout, stderr, exit status) of win with op = {"step", "size", "small"} on the text of a BED file; only complete lines count"""
    lines = text.split("\n")[:-1]
    out = ""
    k = 0
    while k < len(lines) and rr.is_header(lines[k]):                  # hide_header = false (genomic_regions.cpp:702-704)
        out += lines[k] + "\n"
        k += 1
    for n in range(k, len(lines)):
        try:
            out += windows_of(read_bed(lines[n], n + 1), op["step"], op["size"], op["small"])
        except InputError as err:
            return out, err.text, 1
    return out, "", 0


# ---- the closed forms (size >= 1, step >= 1, a plain line) ----------------------------------------------------------------------
def digits(v):
    return len("%d" % v)


def n_full(length, step, size):
    """c: the windows of full size of a line with len = STOP - START + 1"""
    return 0 if size > length else (length - size) // step + 1


def n_windows(length, step, size, small):
    """n: the windows printed"""
    if length <= 0:
        return 0
    return (length - 1) // step + 1 if small else n_full(length, step, size)


def progression_digits(a, d, m):
    """digits(a) + digits(a + d) + .. over m terms, a >= 0, d >= 1, terms below 10^10: m + sum over j = 1..9 of max(0, m - k_j) with
    k_j = 0 when a >= 10^j, else ceil((10^j - a) / d), the first term with more than j digits"""
    total = m
    for j in range(1, 10):
        p = 10 ** j
        kj = 0 if a >= p else (p - a + d - 1) // d
        total += max(0, m - kj)
    return total


def bytes_before(line, step, size, small, k):
    """the bytes of the first k windows of a plain line, k <= n"""
    tok = line.split("\t")
    v2, stop = int(tok[1]), int(tok[2])
    tail = "" if len(tok) == 3 else "\t" + tok[3] if len(tok) < 6 else "\t" + "\t".join(tok[3:])
    fixed = len(tok[0]) + 2 + len(tail) + 1
    c = n_full(stop - v2, step, size)
    full = min(k, c)
    return k * fixed + progression_digits(v2, step, k) + progression_digits(v2 + size, step, full) + (k - full) * digits(stop)


def fixed_part(line):
    """the bytes of a plain line's windows that are no digits of columns 2 and 3: column 1, two tabs, the tail, the newline"""
    tok = line.split("\t")
    tail = "" if len(tok) == 3 else "\t" + tok[3] if len(tok) < 6 else "\t" + "\t".join(tok[3:])
    return len(tok[0]) + 2 + len(tail) + 1
