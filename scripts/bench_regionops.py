#!/usr/bin/env python3
"""genomic_regions' line-based interval operations, measured on one MI355X.

1. The passes alone: one block of n_block plain 6-column lines through gtx_rewrite_text from page-locked memory, `shiftp`
   (everything kept) and `fix` at about half kept, under gtx_profile_enable: the events bracket the plan, prefix and emit launches,
   which run on text that is already in HBM behind its newline index and tokenizer.  Reported: ms, and the fraction of the 8000 GB/s
   peak on text in + newline index (4 B a line) + text out.  Beside it the whole call by the host clock (copy in, index, tokenizer,
   passes, copy of the result back).
2. `genomic_regions shift -start 0 -stop 0` end to end (process start to exit) to a file and to a pipe, beside
   `genomic_subset -inv -i` of the same file against a reference set that matches nothing (the same bytes in and out through the
   same block pump, with a join on top) -- the binary given with --yardstick (a build of the parent commit), else this build's --
   and the host loop (GTX_TEXT_ON_DEVICE=0) on a tenth of the lines.  Medians of 5.
Usage: bench_regionops.py [n_lines] [--block N] [--dir D] [--yardstick PATH-TO-genomic_subset]"""
import os, statistics, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
BIN = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc")
d = sys.argv[sys.argv.index("--dir") + 1] if "--dir" in sys.argv else os.environ.get("TMPDIR", "/tmp")
opt = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 100_000_000
n_block = int(opt("--block") or min(n, 100_000_000))
YARD = opt("--yardstick") or os.path.join(BIN, "genomic_subset")
REPS = 5


def write_reads(path, count, half_invalid=False):
    """plain 6-column lines on 24 chromosomes, position-sorted inside a chromosome; half_invalid: every other line has start > stop"""
    import numpy as np
    rng = np.random.default_rng(3)
    with open(path, "wb") as f:
        left = count
        while left:
            m = min(left, 2_000_000)
            c = rng.integers(1, 25, m); s = rng.integers(0, 100_000_000, m); k = np.arange(m)
            e = s + 50
            if half_invalid:
                e = np.where(k & 1, s - 5, e)
            strand = np.where(rng.integers(0, 2, m) == 1, "+", "-")
            lines = np.char.add(np.char.add(np.char.add("chr", c.astype(str)), "\t"), s.astype(str))
            lines = np.char.add(np.char.add(lines, "\t"), np.maximum(e, 0).astype(str))
            lines = np.char.add(np.char.add(lines, "\tr\t0\t"), strand)
            f.write(("\n".join(lines.tolist()) + "\n").encode())
            left -= m


def passes_alone():
    import ctypes
    import gtx
    e = gtx.Engine(0)
    e.profile(1)
    for name, op, half in (("shiftp -5p 100 -3p 50, all kept", gtx.RewriteOp.make("shiftp", 100, 50), False), ("fix, about half kept", gtx.RewriteOp.make("fix"), True)):
        path = os.path.join(d, "regionops_block.bed")
        write_reads(path, n_block, half)
        text = open(path, "rb").read()
        lines = text.count(b"\n")
        src = e.lib.gtx_host_alloc(e.ctx, len(text)); cap = int(e.lib.gtx_rewrite_max_bytes(len(text), lines))
        dst = e.lib.gtx_host_alloc(e.ctx, cap)
        ctypes.memmove(src, text, len(text))
        walls, kernels, out_bytes = [], [], 0
        for _ in range(REPS + 1):
            t = ctypes.c_int(-1); redo, nb, ns = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_int64(0)
            t0 = time.perf_counter()
            e._chk(e.lib.gtx_rewrite_text(e.ctx, ctypes.c_char_p(src), len(text), lines, ctypes.byref(op), ctypes.byref(t)))
            e._chk(e.lib.gtx_rewrite_result(e.ctx, t.value, ctypes.byref(redo), ctypes.c_void_p(dst), cap, ctypes.byref(nb), ctypes.byref(ns)))
            walls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(e.profile_last()[0])
            assert redo.value == 0
            out_bytes = nb.value
        ms, wall = statistics.median(kernels[1:]), statistics.median(walls[1:])
        moved = len(text) + 4 * lines + out_bytes
        print("%d lines resident in HBM (%.1f MB in, %.1f MB out), %s: plan + prefix + emit %.3f ms (median of %d; %.3f-%.3f), %.0f GB/s on text in + newline index + text out"
              " = %.3f of the 8000 GB/s peak; the whole call from page-locked memory and back %.1f ms"
              % (lines, len(text) / 1e6, out_bytes / 1e6, name, ms, REPS, min(kernels[1:]), max(kernels[1:]), moved / ms / 1e6, moved / ms / 1e6 / 8000, wall))
        e.lib.gtx_host_free(e.ctx, ctypes.c_void_p(src)); e.lib.gtx_host_free(e.ctx, ctypes.c_void_p(dst))
        os.remove(path)
    e.close()


def timed(cmd, env, stdout):
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, env=env, stdout=stdout, shell=isinstance(cmd, str))
    return time.perf_counter() - t0


def end_to_end():
    reads, out, none = os.path.join(d, "regionops_reads.bed"), os.path.join(d, "regionops_out.bed"), os.path.join(d, "regionops_none.bed")
    write_reads(reads, n)
    open(none, "w").write("chrNone\t0\t10\tx\t0\t+\n")
    env = dict(os.environ); env.pop("GTX_TEXT_ON_DEVICE", None)
    size = os.path.getsize(reads)
    tool = [os.path.join(BIN, "genomic_regions"), "shift", "-start", "0", "-stop", "0", reads]
    yard = [YARD, "-inv", "-i", none, reads]
    res = {}
    for name, cmd in (("genomic_regions shift -start 0 -stop 0", tool), ("genomic_subset -inv -i (nothing matches)", yard)):
        to_file = statistics.median(timed(cmd, env, open(out, "wb")) for _ in range(REPS))
        same = open(out, "rb").read(1 << 20) == open(reads, "rb").read(1 << 20) and os.path.getsize(out) == size
        to_pipe = statistics.median(timed(" ".join(cmd) + " | cat > /dev/null", env, None) for _ in range(REPS))
        res[name] = (to_file, to_pipe)
        print("%-45s %d lines, %.0f MB: to a file %.3f s, to a pipe %.3f s (medians of %d; output %s the input)" % (name, n, size / 1e6, to_file, to_pipe, REPS, "equals" if same else "DIFFERS FROM"))
    a, b = res["genomic_regions shift -start 0 -stop 0"], res["genomic_subset -inv -i (nothing matches)"]
    print("yardstick binary: %s" % ("this build's" if YARD.startswith(BIN) else "a build of the parent commit"))
    print("ratio to the yardstick: to a file %.2f, to a pipe %.2f (acceptance: no worse than 1.15: %s)" % (a[0] / b[0], a[1] / b[1], "met" if max(a[0] / b[0], a[1] / b[1]) <= 1.15 else "MISSED"))
    small = os.path.join(d, "regionops_small.bed")
    write_reads(small, max(n // 10, 1))
    env0 = dict(env, GTX_TEXT_ON_DEVICE="0")
    t = statistics.median(timed([tool[0]] + tool[1:-1] + [small], env0, open(out, "wb")) for _ in range(3))
    print("host loop (GTX_TEXT_ON_DEVICE=0) on %d lines: %.2f s to a file (median of 3), %.2f M lines/s" % (max(n // 10, 1), t, max(n // 10, 1) / t / 1e6))
    for f in (reads, out, none, small):
        os.remove(f)


if __name__ == "__main__":
    passes_alone()
    end_to_end()
