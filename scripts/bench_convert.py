#!/usr/bin/env python3
"""genomic_convert bed on SAM reads, measured on one MI355X: n reads of 100 bp (gtx_packtool synthsam: 267 B a line, the shape of
profiles/sam_bench.txt).

1. The passes alone: the file in blocks of 64 MB through gtx_convert_text / gtx_convert_result from page-locked memory under
   gtx_profile_enable.  The events bracket the plan, prefix and emit launches of every block, on text that is already in HBM behind
   its newline index and tokenizer.  Reported: their ms summed over the blocks and the fraction of the 8000 GB/s peak on text in +
   newline index + text out.  With --trace, one run of the tool under `rocprofv3 --kernel-trace --stats`: the tokenizer's parse
   kernel beside the plan and emit kernels, on the same blocks in the same run.
2. The tool end to end (process start to exit), medians of 5, to a file and to a pipe: the device path beside this build's host loop
   (GTX_TEXT_ON_DEVICE=0), and beside `genomic_overlaps count -S -i` on the same SAM file against a one-region reference, which reads
   the same bytes through the same tokenizer and writes nothing; and 1000 reads, the fixed cost of going to the device.
Usage: bench_convert.py [n_reads] [--dir D] [--only passes,tool] [--reps N] [--trace]"""
import csv, ctypes, glob, os, shutil, statistics, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
BIN = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc")
opt = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
d = opt("--dir") or os.environ.get("TMPDIR", "/tmp")
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10_000_000
ONLY = (opt("--only") or "passes,tool").split(",")
REPS = int(opt("--reps") or 5)
BLOCK = 64 << 20
TOOL, OVERLAPS = os.path.join(BIN, "genomic_convert"), os.path.join(BIN, "genomic_overlaps")


def synth(count, path):
    subprocess.run([os.path.join(BIN, "gtx_packtool"), "synthsam", str(count), "44", path, "100"], check=True)
    return os.path.getsize(path)


def blocks_of(path):
    """the file's data lines in blocks of complete lines of at most BLOCK bytes"""
    text = open(path, "rb").read()
    at = 0
    while text.startswith(b"@", at):
        at = text.index(b"\n", at) + 1
    out = []
    while at < len(text):
        end = len(text) if len(text) - at <= BLOCK else text.rindex(b"\n", at, at + BLOCK) + 1
        out.append(text[at:end]); at = end
    return out


def passes_alone(path):
    import gtx
    e = gtx.Engine(0)
    op = gtx.ConvertOp.make("bed")
    blocks = blocks_of(path)
    assert len(blocks) < 63, "more blocks than the profile ring keeps"
    cap = max(int(e.lib.gtx_convert_max_bytes(len(b), b.count(b"\n"), ctypes.byref(op))) for b in blocks)
    src, dst = e.lib.gtx_host_alloc(e.ctx, BLOCK), e.lib.gtx_host_alloc(e.ctx, cap)
    runs, walls, total_out = [], [], 0
    for rep in range(REPS + 1):
        e.profile(1)                                                   # (resets the ring: what is read back below is this repetition's)
        t0 = time.perf_counter(); total_out = 0
        for b in blocks:
            ctypes.memmove(src, b, len(b))
            t, redo, nb = ctypes.c_int(-1), ctypes.c_int(0), ctypes.c_size_t(0)
            e._chk(e.lib.gtx_convert_text(e.ctx, ctypes.c_char_p(src), len(b), b.count(b"\n"), ctypes.byref(op), gtx.TEXT_SAM, ctypes.byref(t)))
            e._chk(e.lib.gtx_convert_result(e.ctx, t.value, ctypes.byref(redo), ctypes.c_void_p(dst), cap, ctypes.byref(nb), None))
            assert redo.value == 0
            total_out += nb.value
        walls.append((time.perf_counter() - t0) * 1e3)
        assert e.profiled_calls() == len(blocks)
        runs.append(sum(e.profile_last(back)[0] for back in range(len(blocks))))
    ms = statistics.median(runs[1:])
    size, lines = sum(len(b) for b in blocks), sum(b.count(b"\n") for b in blocks)
    moved = size + 4 * lines + total_out
    print("%d reads of 100 bp (%.1f MB in, %d blocks, %.1f MB out): plan + prefix + emit %.3f ms summed over the blocks (median of %d; %.3f-%.3f), "
          "%.0f GB/s on text in + newline index + text out = %.3f of the 8000 GB/s peak; %.0f GB/s of text in; the blocks one after the other "
          "from page-locked memory, each copied back, %.0f ms by the host clock"
          % (lines, size / 1e6, len(blocks), total_out / 1e6, ms, REPS, min(runs[1:]), max(runs[1:]), moved / ms / 1e6, moved / ms / 1e6 / 8000, size / ms / 1e6, statistics.median(walls[1:])))
    for p in (src, dst):
        e.lib.gtx_host_free(e.ctx, ctypes.c_void_p(p))
    e.close()


def kernel_trace(path):
    if not shutil.which("rocprofv3"):
        print("rocprofv3 is not on the path: no kernel trace"); return
    od = os.path.join(d, "convert_prof")
    shutil.rmtree(od, ignore_errors=True)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", od, "-o", "run", "--", TOOL, "bed", path],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
    if r.returncode != 0:
        sys.exit("the profiled run failed (rc %d): %s" % (r.returncode, r.stderr.decode()[-2000:]))
    stats = glob.glob(os.path.join(od, "**", "*kernel_stats.csv"), recursive=True)
    size = os.path.getsize(path)
    for row in csv.DictReader(open(stats[0])) if stats else ():
        if any(x in row["Name"] for x in ("text_parse_kernel", "nl_", "convert_", "tile_prefix", "text_void")):
            ns = float(row["TotalDurationNs"])
            print("%-72s calls %5s  total %9.3f ms  %8.2f GB/s of text" % (row["Name"][:72], row["Calls"], ns / 1e6, size / ns), flush=True)
    shutil.rmtree(od, ignore_errors=True)


def timed(cmd, env, stdout):
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, env=env, stdout=stdout, shell=isinstance(cmd, str))
    return time.perf_counter() - t0


def end_to_end(name, path, reps, with_count):
    out = os.path.join(d, "convert_out.bed")
    env = dict(os.environ); env.pop("GTX_TEXT_ON_DEVICE", None)
    cmd = [TOOL, "bed", path]
    res = {}
    for way, e in (("device", env), ("host loop", dict(env, GTX_TEXT_ON_DEVICE="0"))):
        to_file = statistics.median(timed(cmd, e, open(out, "wb")) for _ in range(reps))
        size = os.path.getsize(out)
        to_pipe = statistics.median(timed(" ".join(cmd) + " | cat > /dev/null", e, None) for _ in range(reps))
        res[way] = (to_file, to_pipe, size)
        print("%-18s %-10s %.1f MB out: to a file %.3f s, to a pipe %.3f s (medians of %d)" % (name, way, size / 1e6, to_file, to_pipe, reps), flush=True)
    a, b = res["device"], res["host loop"]
    print("%-18s device / host loop: to a file %.2f, to a pipe %.2f%s" % (name, a[0] / b[0], a[1] / b[1], "" if a[2] == b[2] else "  OUTPUT SIZES DIFFER"))
    if with_count:
        ref = os.path.join(d, "convert_ref.bed")
        open(ref, "w").write("chr1\t1000000\t2000000\n")
        cnt = statistics.median(timed([OVERLAPS, "count", "-S", "-i", ref, path], dict(env, GTX_TEXT_ON_DEVICE="1"), subprocess.DEVNULL) for _ in range(reps))
        print("%-18s genomic_overlaps count -S -i against one region, the text tokenised on the device: %.3f s (median of %d); convert / count: to a file %.2f, to a pipe %.2f"
              % (name, cnt, reps, a[0] / cnt, a[1] / cnt))
        os.remove(ref)
    os.remove(out)


if __name__ == "__main__":
    sam = os.path.join(d, "convert_reads.sam")
    size = synth(n, sam)
    print("input: %d reads of 100 bp, %.3f GB, %.0f B a line" % (n, size / 1e9, size / n), flush=True)
    if "passes" in ONLY:
        passes_alone(sam)
        if "--trace" in sys.argv:
            kernel_trace(sam)
    if "tool" in ONLY:
        small = os.path.join(d, "convert_reads_1000.sam")
        synth(1000, small)
        end_to_end("1000 reads", small, REPS, False)
        end_to_end("%d reads" % n, sam, REPS, True)
        os.remove(small)
    os.remove(sam)
