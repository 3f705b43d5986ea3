#!/usr/bin/env python3
"""genomic_windows (genomic_regions win), measured on one MI355X, on two inputs: `genome`, 24 chromosome lines of human size with
-s 500 -d 25 (124 M windows, 2.95 GB of output from 0.5 KB of input), and `reads`, n plain 6-column reads of 50 bp with -s 25 -d 25
(two windows a line).

1. The passes alone: the input as one block through gtx_windows_text / gtx_windows_result from page-locked memory under
   gtx_profile_enable.  The events bracket the plan, prefix and base launches of the block and the emit launch of every range, all
   on text that is already in HBM behind its newline index and tokenizer; the sink drops the text.  Reported: ms of the plan, ms of
   the emit launches together, and the fraction of the 8000 GB/s peak on the bytes written -- to be read beside the 0.20 that
   gtx_window_lines reaches at 100 % kept (profiles/scan_lines_bench.txt), whose emit pass does the same kind of work.  Beside it the
   whole call by the host clock (copy in, index, tokenizer, passes, copies of the ranges back).
2. The tool end to end (process start to exit), medians of 5, to a file and to a pipe, the device path beside this build's host
   loop (GTX_TEXT_ON_DEVICE=0), the only other implementation there is; and 1000 reads, the fixed cost of going to the device.
Usage: bench_windows.py [n_reads] [--dir D] [--only passes,reads,genome] [--reps N]"""
import ctypes, os, statistics, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
BIN = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc")
opt = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
d = opt("--dir") or os.environ.get("TMPDIR", "/tmp")
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10_000_000
ONLY = (opt("--only") or "passes,reads,genome").split(",")
REPS = int(opt("--reps") or 5)
HG19 = [249250621, 243199373, 198022430, 191154276, 180915260, 171115067, 159138663, 146364022, 141213431, 135534747, 135006516, 133851895,
        115169878, 107349540, 102531392, 90354753, 81195210, 78077248, 59128983, 63025520, 48129895, 51304566, 155270560, 59373566]
GENOME = "".join("chr%s\t0\t%d\n" % (c, ln) for c, ln in zip([str(k) for k in range(1, 23)] + ["X", "Y"], HG19))
CHUNK = 256 << 20                                                      # bytes of bound a range: the genome's 2.95 GB in fewer ranges than the profile ring keeps


def reads_text(count, made={}):
    """plain 6-column reads of 50 bp on 24 chromosomes"""
    if count not in made:
        made[count] = make_reads(count)
    return made[count]


def make_reads(count):
    import numpy as np
    rng = np.random.default_rng(3)
    parts, left = [], count
    while left:
        m = min(left, 2_000_000)
        c = rng.integers(1, 25, m); s = rng.integers(0, 100_000_000, m)
        strand = np.where(rng.integers(0, 2, m) == 1, "+", "-")
        lines = np.char.add(np.char.add(np.char.add("chr", c.astype(str)), "\t"), s.astype(str))
        lines = np.char.add(np.char.add(lines, "\t"), (s + 50).astype(str))
        lines = np.char.add(np.char.add(lines, "\tr\t0\t"), strand)
        parts.append(("\n".join(lines.tolist()) + "\n").encode())
        left -= m
    return b"".join(parts)


def passes_alone():
    import gtx
    e = gtx.Engine(0)
    e.set_lines_chunk(CHUNK)
    drop = gtx.LINES_SINK(lambda user, text, nb: 0)
    for name, text, op in (("genome, 24 lines, -s 500 -d 25", GENOME.encode(), gtx.WindowsOp.make(500, 25)), ("%d reads of 50 bp, -s 25 -d 25" % n, reads_text(n), gtx.WindowsOp.make(25, 25))):
        lines = text.count(b"\n")
        src = e.lib.gtx_host_alloc(e.ctx, len(text))
        ctypes.memmove(src, text, len(text))
        walls, plans, emits, ranges, nw, nb = [], [], [], 0, ctypes.c_int64(0), ctypes.c_int64(0)
        for _ in range(REPS + 1):
            e.profile(1)                                               # (resets the ring: what is read back below is this call's)
            t = ctypes.c_int(-1); redo = ctypes.c_int(0)
            t0 = time.perf_counter()
            e._chk(e.lib.gtx_windows_text(e.ctx, ctypes.c_char_p(src), len(text), lines, ctypes.byref(op), ctypes.byref(t)))
            e._chk(e.lib.gtx_windows_result(e.ctx, t.value, ctypes.byref(redo), drop, None, ctypes.byref(nw), ctypes.byref(nb)))
            walls.append((time.perf_counter() - t0) * 1e3)
            assert redo.value == 0
            ranges = e.profiled_calls() - 1
            assert 0 < ranges < 63, "more ranges than the profile ring keeps: raise CHUNK"
            emits.append(sum(e.profile_last(back)[0] for back in range(ranges)))
            plans.append(e.profile_last(ranges)[0])
        plan, emit, wall = statistics.median(plans[1:]), statistics.median(emits[1:]), statistics.median(walls[1:])
        print("%s (%.1f MB in, %d windows, %.1f MB out in %d ranges): plan + prefixes + bases %.3f ms, emit %.3f ms (medians of %d; emit %.3f-%.3f), "
              "%.0f GB/s on the bytes written = %.3f of the 8000 GB/s peak (gtx_window_lines at 100 %% kept: 0.20); the whole call from page-locked memory "
              "with the ranges copied back %.1f ms"
              % (name, len(text) / 1e6, nw.value, nb.value / 1e6, ranges, plan, emit, REPS, min(emits[1:]), max(emits[1:]), nb.value / (plan + emit) / 1e6,
                 nb.value / (plan + emit) / 1e6 / 8000, wall))
        e.lib.gtx_host_free(e.ctx, ctypes.c_void_p(src))
    e.close()


def timed(cmd, env, stdout):
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, env=env, stdout=stdout, shell=isinstance(cmd, str))
    return time.perf_counter() - t0


def end_to_end(name, text, args, reps):
    src, out = os.path.join(d, "windows_in.bed"), os.path.join(d, "windows_out.bed")
    open(src, "wb").write(text)
    env = dict(os.environ); env.pop("GTX_TEXT_ON_DEVICE", None)
    cmd = [os.path.join(BIN, "genomic_windows")] + args + [src]
    res = {}
    for way, e in (("device", env), ("host loop", dict(env, GTX_TEXT_ON_DEVICE="0"))):
        to_file = statistics.median(timed(cmd, e, open(out, "wb")) for _ in range(reps))
        size = os.path.getsize(out)
        to_pipe = statistics.median(timed(" ".join(cmd) + " | cat > /dev/null", e, None) for _ in range(reps))
        res[way] = (to_file, to_pipe, size)
        print("%-28s %-10s %.1f MB out: to a file %.3f s, to a pipe %.3f s (medians of %d)" % (name, way, size / 1e6, to_file, to_pipe, reps))
    a, b = res["device"], res["host loop"]
    print("%-28s device / host loop: to a file %.2f, to a pipe %.2f%s" % (name, a[0] / b[0], a[1] / b[1], "" if a[2] == b[2] else "  OUTPUT SIZES DIFFER"))
    for f in (src, out):
        os.remove(f)


if __name__ == "__main__":
    if "passes" in ONLY:
        passes_alone()
    if "reads" in ONLY:
        end_to_end("1000 reads -s 25 -d 25", reads_text(1000), ["-s", "25", "-d", "25"], REPS)
        end_to_end("%d reads -s 25 -d 25" % n, reads_text(n), ["-s", "25", "-d", "25"], REPS)
    if "genome" in ONLY:
        end_to_end("genome -s 500 -d 25", GENOME.encode(), ["-s", "500", "-d", "25"], REPS)
