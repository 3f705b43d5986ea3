"""Inputs of the sliding windows' CPU tests (test_windows_cli_cpu.py, test_windows_caller_cpu.py): seeded BED lines, plain ones mixed
with lines only the host loop takes, and the options they are run with -- among them steps and sizes beyond 2^31 and 2^62, which
the loop must take without overflow, and a size below 1."""
import numpy as np


def seeded_lines(seed, n=3000, error_line=True):
    """mixed plain and odd lines on three chromosomes; a multi-block BED12 line last"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        c = "chr%d" % rng.integers(1, 4)
        s = int(rng.integers(0, 2_000_000)); ln = int(rng.integers(-5, 400))
        cols = [c, str(s), str(max(s + ln, 0)), "r%d" % k, str(int(rng.integers(-5, 1000))), "+-"[int(rng.integers(0, 2))]]
        kind = int(rng.integers(0, 12))
        if kind < 6:
            line = "\t".join(cols[:int(rng.integers(3, 7))])                       # plain, 3 to 6 columns
        elif kind == 6:
            line = " ".join(cols[:int(rng.integers(3, 7))])                        # space-separated
        elif kind == 7:
            line = "\t".join(cols[:5] + [[".", "1", "-1"][int(rng.integers(0, 3))]])
        elif kind == 8:
            line = "\t".join([c, "00%d" % s, "+%d" % (s + ln), cols[3], "007", "+"])   # leading zeros, a sign, a score that is not canonical
        elif kind == 9:
            line = "\t".join(cols + [str(s + 5)])                                  # 7 columns: six are printed
        elif kind == 10:
            line = "\t".join(cols + [str(s + 5), str(s + 9), "255,0,0"][:int(rng.integers(2, 4))])
        else:                                                                     # BED12 with one block
            line = "\t".join([c, str(s), str(s + 50), cols[3], cols[4], cols[5], str(s), str(s + 50), "0", "1", "50,", "0,"])
        out.append(line)
    if error_line:
        out.append("chr1\t10\t50\tt\t0\t+\t10\t50\t0\t2\t10,10,\t0,30,")
        out.append("chr1\t0\t100")
    return "".join(l + "\n" for l in out)


OPS = [{"step": 25, "size": 25, "small": False}, {"step": 10, "size": 100, "small": True}, {"step": 1, "size": 1, "small": False},
       {"step": 7, "size": 30, "small": False}, {"step": 2 ** 33, "size": 3, "small": True}, {"step": 50, "size": 2 ** 40, "small": True},
       {"step": 3, "size": 0, "small": False}, {"step": 2 ** 62, "size": 2 ** 63 - 1, "small": True}]
