#!/usr/bin/env python3
"""genomic_blocks on BED12 text, measured on one MI355X, on two inputs: a synthetic annotation of n_annot transcripts (block counts
drawn with a mean of about 10 and a tail to 400, lists with trailing commas, sorted by position) and n_reads spliced reads of 1 to 3
blocks (`bamToBed -bed12`).  Both are 50 000 / 100 000 seeded lines repeated to the size asked for.

Condition, not a measurement: every block of every operation is rendered on the device -- the script asserts zero needs_host blocks
in the passes and zero blocks that came back in the tool's GTX_TEXT_TRACE line, and prints the counts.

1. The passes alone, per operation: the file in blocks of 64 MB through gtx_blocks_text / gtx_blocks_result from page-locked memory
   under gtx_profile_enable.  The events bracket the plan and prefix launches (gtx_blocks_text) and the emit launch
   (gtx_blocks_result) of every block, on text that is already in HBM behind its newline index.  Reported: their ms summed over the
   blocks and the fraction of the 8000 GB/s peak on text in + newline index + text out.
2. The tool end to end (process start to exit), medians of --reps (5), to a file and to a pipe; beside it this build's host loop
   (GTX_TEXT_ON_DEVICE=0) and `genomic_regions fix` on the same file, the one-core loop that prints the same Print line for every
   BED12 line and is all there was for such a file before genomic_blocks (--host-reps, 1: they take seconds each); and 1000 lines,
   the fixed cost of going to the device.
Usage: bench_blocks.py [n_annot] [n_reads] [--dir D] [--only passes,tool] [--reps N] [--host-reps N]"""
import ctypes, os, random, re, statistics, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
BIN = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc")
opt = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
d = opt("--dir") or os.environ.get("TMPDIR", "/tmp")
nums = [int(a) for a in sys.argv[1:3] if a.isdigit()]
N_ANNOT, N_READS = (nums + [1_000_000, 10_000_000][len(nums):])[:2]
ONLY = (opt("--only") or "passes,tool").split(",")
REPS, HOST_REPS = int(opt("--reps") or 5), int(opt("--host-reps") or 1)
BLOCK = 64 << 20
TOOL, REGIONS = os.path.join(BIN, "genomic_blocks"), os.path.join(BIN, "genomic_regions")
OPS = [("split", []), ("connect", []), ("select", ["-5p"]), ("diff", []), ("n", []), ("strand", ["-op", "r"])]
TRACE = re.compile(r"\[gtx blocks\] blocks rendered on the device: (\d+), came back: (\d+)")


def bed12(rng, chrom, at, name, n):
    sizes, starts, p = [], [], 0
    for k in range(n):
        if k:
            p += rng.randint(1, 3000)
        s = rng.randint(20, 400)
        sizes.append(s); starts.append(p); p += s
    return "%s\t%d\t%d\t%s\t0\t%s\t%d\t%d\t0\t%d\t%s,\t%s,\n" % (chrom, at, at + p, name, rng.choice("+-"), at + starts[0] + 5, at + p - 5, n,
                                                                    ",".join(map(str, sizes)), ",".join(map(str, starts)))


def annotation(rng, count):
    """transcripts in position order: 1 to 30 exons mostly, one in 200 with 100 to 400 (mean about 10)"""
    out, at = [], 10_000
    for k in range(count):
        n = rng.randint(100, 400) if rng.random() < 0.005 else max(1, min(60, int(rng.expovariate(1 / 8.0)) + 1))
        at += rng.randint(0, 20_000)
        out.append(bed12(rng, "chr%d" % (1 + k * 22 // count), at % 200_000_000, "ENST%011d.%d" % (k, 1 + k % 9), n))
    return out


def reads(rng, count):
    out, at = [], 10_000
    for k in range(count):
        at += rng.randint(0, 400)
        out.append(bed12(rng, "chr%d" % (1 + k * 22 // count), at % 200_000_000, "read%08d/1" % k, rng.choice((1, 1, 2, 2, 2, 3))))
    return out


def write_repeated(path, lines, total):
    text = "".join(lines)
    with open(path, "w") as f:
        for _ in range(total // len(lines)):
            f.write(text)
        f.write("".join(lines[:total % len(lines)]))
    return os.path.getsize(path)


def blocks_of(path):
    """the file in blocks of complete lines of at most BLOCK bytes"""
    text = open(path, "rb").read()
    at, out = 0, []
    while at < len(text):
        end = len(text) if len(text) - at <= BLOCK else text.rindex(b"\n", at, at + BLOCK) + 1
        out.append(text[at:end]); at = end
    return out


def passes_alone(name, path):
    import gtx
    e = gtx.Engine(0)
    blocks = blocks_of(path)
    assert 2 * len(blocks) < 63, "more blocks than the profile ring keeps"
    src = e.lib.gtx_host_alloc(e.ctx, BLOCK)
    size, lines = sum(len(b) for b in blocks), sum(b.count(b"\n") for b in blocks)
    taken = [0]

    def take(user, p, n):
        taken[0] += n
        return 0
    sink = gtx.LINES_SINK(take)
    for word, args in OPS:
        op = gtx.BlocksOp.make(word, gtx.BLOCKS_5P if word == "select" else 0, "r")
        runs, back_to_host, total_out = [], 0, 0
        for rep in range(REPS + 1):
            e.profile(1)                                               # (resets the ring: what is read back below is this repetition's)
            taken[0] = 0
            for b in blocks:
                ctypes.memmove(src, b, len(b))
                t, redo = ctypes.c_int(-1), ctypes.c_int(0)
                e._chk(e.lib.gtx_blocks_text(e.ctx, ctypes.c_char_p(src), len(b), b.count(b"\n"), ctypes.byref(op), ctypes.byref(t)))
                e._chk(e.lib.gtx_blocks_result(e.ctx, t.value, ctypes.byref(redo), sink, None, None, None))
                back_to_host += redo.value != 0
            total_out = taken[0]
            calls = e.profiled_calls()
            assert calls == 2 * len(blocks), calls
            runs.append(sum(e.profile_last(back)[0] for back in range(calls)))
        assert back_to_host == 0, "%s %s: %d needs_host blocks" % (name, word, back_to_host)
        ms = statistics.median(runs[1:])
        moved = size + 4 * lines + total_out
        print("%-10s %-8s %d lines (%.1f MB in, %d blocks, %.1f MB out), needs_host blocks 0: plan + prefix + emit %.3f ms summed over the blocks "
              "(median of %d; %.3f-%.3f), %.0f GB/s on text in + newline index + text out = %.3f of the 8000 GB/s peak; %.0f GB/s of text in"
              % (name, word, lines, size / 1e6, len(blocks), total_out / 1e6, ms, REPS, min(runs[1:]), max(runs[1:]), moved / ms / 1e6, moved / ms / 1e6 / 8000, size / ms / 1e6), flush=True)
    e.lib.gtx_host_free(e.ctx, ctypes.c_void_p(src))
    e.close()


def timed(cmd, env, stdout, stderr=None):
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, env=env, stdout=stdout, stderr=stderr, shell=isinstance(cmd, str))
    return time.perf_counter() - t0


def end_to_end(name, path, ops, with_fix):
    out = os.path.join(d, "blocks_out.txt")
    env = dict(os.environ); env.pop("GTX_TEXT_ON_DEVICE", None)
    host = dict(env, GTX_TEXT_ON_DEVICE="0")
    for word, args in ops:
        cmd = [TOOL, word] + args + [path]
        r = subprocess.run(cmd, env=dict(env, GTX_TEXT_TRACE="1"), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, check=True)
        m = TRACE.search(r.stderr.decode())
        assert m and int(m.group(2)) == 0, "%s %s: %s" % (name, word, r.stderr.decode()[-300:])
        to_file = statistics.median(timed(cmd, env, open(out, "wb")) for _ in range(REPS))
        size = os.path.getsize(out)
        to_pipe = statistics.median(timed(" ".join(cmd) + " | cat > /dev/null", env, None) for _ in range(REPS))
        loop = statistics.median(timed(cmd, host, open(out, "wb")) for _ in range(HOST_REPS))
        same = os.path.getsize(out) == size
        print("%-10s %-8s blocks on the device %s, came back 0; %.1f MB out: to a file %.3f s, to a pipe %.3f s (medians of %d); host loop to a file %.3f s "
              "(median of %d); device / host loop %.2f%s" % (name, word, m.group(1), size / 1e6, to_file, to_pipe, REPS, loop, HOST_REPS, to_file / loop, "" if same else "  OUTPUT SIZES DIFFER"), flush=True)
    if with_fix:
        fix = statistics.median(timed([REGIONS, "fix", path], host, open(out, "wb")) for _ in range(HOST_REPS))
        print("%-10s genomic_regions fix, the one-core loop printing every line again: to a file %.3f s (median of %d)" % (name, fix, HOST_REPS), flush=True)
    os.remove(out)


if __name__ == "__main__":
    rng = random.Random(77)
    inputs = []
    for name, make, distinct, total in (("annotation", annotation, 50_000, N_ANNOT), ("reads", reads, 100_000, N_READS)):
        lines = make(rng, min(distinct, total))
        path = os.path.join(d, "blocks_%s.bed" % name)
        size = write_repeated(path, lines, total)
        counts = [int(l.split("\t")[9]) for l in lines]
        print("input %s: %d lines, %.3f GB, %.0f B a line, %.1f blocks a line on average, %d at most" % (name, total, size / 1e9, size / total, sum(counts) / len(counts), max(counts)), flush=True)
        inputs.append((name, path, lines))
    if "passes" in ONLY:
        for name, path, _ in inputs:
            passes_alone(name, path)
    if "tool" in ONLY:
        small = os.path.join(d, "blocks_1000.bed")
        open(small, "w").write("".join(inputs[1][2][:1000]))
        end_to_end("1000 reads", small, OPS[:1] + OPS[-1:], False)
        os.remove(small)
        for name, path, _ in inputs:
            end_to_end(name, path, OPS, True)
    for _, path, _ in inputs:
        os.remove(path)
