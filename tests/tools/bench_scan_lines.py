#!/usr/bin/env python3
"""The line renderer of `genomic_scans counts` (gtx_window_lines_device, csrc/gtx_lines.hip), measured on one MI355X.

Part 1, the pass alone: a synthetic window vector in HBM (Poisson counts around 3, as bench_peaks.py makes them) over the stranded
layout of a human-size genome at -w 500 -d 25 (248 M windows), min_value 13, 8, 3 and 0: about 0.002 %, 1.2 %, 58 % and 100 % of the
windows kept.  Per shape the device entry over the whole vector (count, two prefix scans, emit and the read-back of the totals; HIP
events around the call, one warm-up, median of 5), its algorithmic bytes -- 8 B read per window plus the text written -- as a share of
the HBM peak bench.py's `roofline` uses, and beside it gtx_window_select without controls on the same vector at the same threshold:
the pass it extends.
Part 2, end to end: `genomic_scans counts -w 500 -d 25` on --e2e BED reads over that genome at -min 10 and -min 0, stdout to a file and
to a pipe that a reader drains, process start to exit and peak host memory, --runs runs each of this tree's tool and of the tool under
--parent DIR (a second build, its libgtx.so beside it), alternating; medians and ranges, and the rule of the default: the device path
stays the default only if its median is at or under the parent's median plus the parent's own range for every shape.  One more run of
this tree's tool per -min with GTX_LINES_TIMING=1 says where the host waited: for the passes, for the copies, in the sink.
Usage: bench_scan_lines.py [--windows N | --windows 0] [--e2e N | --e2e 0] [--runs K] [--parent DIR] [--dir D]"""
import hashlib, os, subprocess, sys, threading, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
flag_val = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
d = flag_val("--dir") or os.environ.get("TMPDIR", "/tmp")
REPS = 5
HBM_PEAK_GBS = 8000.0                                                     # bench.py's roofline peak
# human chromosomes 1..22, X, Y (GRCh38, rounded to kb)
HUMAN = [248956, 242193, 198295, 190214, 181538, 170805, 159345, 145138, 138394, 133797, 135086, 133275, 114364, 107043, 101991, 90338, 83257,
         80373, 58617, 64444, 46709, 50818, 156040, 57227]
NAMES = ["chr%s" % x for x in list(range(1, 23)) + ["X", "Y"]]
STEP, SIZE = 25, 500


def event_ms(fn):
    """HIP events around fn on the stream the context uses (the null stream): one warm-up, the median and the minimum of REPS"""
    import torch
    fn()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2], min(ts)


def part1(n_cap):
    import numpy as np, torch, gtx
    dev = torch.device("cuda:0")
    e = gtx.Engine(0)
    order = sorted(range(len(NAMES)), key=lambda k: NAMES[k])            # the scanner's blocks: chromosomes in strcmp order, '+' then '-'
    off, names, strands = [0], [], ""
    for k in order:
        for s in "+-":
            nw = gtx.load().gtx_scan_n_windows(HUMAN[k] * 1000, STEP, SIZE)
            if off[-1] + nw > n_cap:
                nw = max(n_cap - off[-1], 0)
            off.append(off[-1] + nw); names.append(NAMES[k]); strands += s
    n = off[-1]
    mb = e.lines_layout(off, names, strands, STEP, SIZE)
    g = torch.Generator(device=dev); g.manual_seed(7)
    S = torch.poisson(torch.full((n,), 3.0, device=dev), generator=g).to(torch.int64)
    text = torch.empty(n * mb, dtype=torch.uint8, device=dev)
    print("%d windows in %d blocks (%.2f GB), longest line %d B, text buffer %.2f GB, tile %d, REPS %d" % (n, len(names), n * 8 / 1e9, mb, n * mb / 1e9, gtx.LINES_TILE, REPS), flush=True)
    for min_value in (13, 8, 3, 0):
        call = lambda: e.window_lines_device(S.data_ptr(), 0, n, n, min_value, text.data_ptr(), n * mb)
        lines, nbytes, end = call()
        assert end == -1 and lines == int((S >= min_value).sum().item())
        med, lo = event_ms(call)
        moved = n * 8.0 + nbytes
        cap = lines + 1
        d_o = torch.empty(cap, dtype=torch.int64, device=dev); d_r32 = torch.empty(cap, dtype=torch.int32, device=dev)
        sel = lambda: e.window_select([S.data_ptr()], [np.array([min_value], dtype=np.int32)], 1 << 30, n_windows=n, capacity=cap, device_out=(d_o.data_ptr(), d_r32.data_ptr()))
        assert sel() == lines
        s_med, s_lo = event_ms(sel)
        del d_o, d_r32
        head = text[:200].cpu().numpy().tobytes().split(b"\n")[0].decode()
        print("  min_value %2d: %d lines (%.4f %%), %.3f GB of text | lines %.3f ms (min %.3f) for %.3f GB = %.0f GB/s = %.2f of the %.0f GB/s peak | "
              "gtx_window_select, no controls: %.3f ms (min %.3f) | lines / select = %.2f | first line %r"
              % (min_value, lines, 100.0 * lines / n, nbytes / 1e9, med, lo, moved / 1e9, moved / med / 1e6, moved / med / 1e6 / HBM_PEAK_GBS, HBM_PEAK_GBS, s_med, s_lo, med / s_med, head), flush=True)
    e.close()


def run_tool(tool, args, to_pipe, out, env, want_md5):
    """process start to exit -> (seconds, peak host GB, rc, bytes of stdout, md5 or None)"""
    t0 = time.perf_counter()
    if to_pipe:
        pr = subprocess.Popen([tool] + args, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env)
        got = [0]
        def drain():
            while True:
                b = pr.stdout.read(1 << 22)
                if not b:
                    break
                got[0] += len(b)
        th = threading.Thread(target=drain); th.start()
        _, status, ru = os.wait4(pr.pid, 0)
        th.join()
        dt = time.perf_counter() - t0
        return dt, ru.ru_maxrss / 1e6, os.waitstatus_to_exitcode(status), got[0], None
    with open(out, "wb") as f:
        pr = subprocess.Popen([tool] + args, stdout=f, stderr=subprocess.DEVNULL, env=env)
        _, status, ru = os.wait4(pr.pid, 0)
    dt = time.perf_counter() - t0
    if not want_md5:
        return dt, ru.ru_maxrss / 1e6, os.waitstatus_to_exitcode(status), os.path.getsize(out), None
    h = hashlib.md5()
    with open(out, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return dt, ru.ru_maxrss / 1e6, os.waitstatus_to_exitcode(status), os.path.getsize(out), h.hexdigest()[:12]


def part2(n_reads, runs, parent):
    import numpy as np
    rng = np.random.default_rng(11)
    lengths = np.asarray(HUMAN, dtype=np.int64) * 1000
    genome, reads, out = os.path.join(d, "lines_genome.bed"), os.path.join(d, "lines_reads.bed"), os.path.join(d, "lines.out")
    with open(genome, "w") as f:
        f.write("".join("%s\t0\t%d\n" % (nm, ln) for nm, ln in zip(NAMES, lengths)))
    t0 = time.perf_counter()
    c = rng.choice(len(NAMES), size=n_reads, p=lengths / lengths.sum())
    s = (rng.random(n_reads) * (lengths[c] - 37)).astype(np.int64)
    pk = rng.integers(0, n_reads, size=5000)                               # half of the reads in 5000 peaks of 2 kb
    k = rng.integers(0, 5000, size=n_reads // 2)
    c[:n_reads // 2] = c[pk][k]; s[:n_reads // 2] = np.maximum(s[pk][k] + rng.integers(-1000, 1000, size=n_reads // 2), 0)
    m = rng.integers(0, 2, size=n_reads)
    with open(reads, "w") as f:
        for lo in range(0, n_reads, 1 << 20):
            hi = min(n_reads, lo + (1 << 20))
            f.write("".join("%s\t%d\t%d\tr\t0\t%s\n" % (NAMES[a], b, b + 36, "+-"[y]) for a, b, y in zip(c[lo:hi].tolist(), s[lo:hi].tolist(), m[lo:hi].tolist())))
    print("e2e: %d reads written in %.1f s" % (n_reads, time.perf_counter() - t0), flush=True)
    tools = [("this tree", os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_scans"))]
    if parent:
        tools.append(("parent", os.path.join(parent, "genomic_scans")))
    env = {k: v for k, v in os.environ.items() if k not in ("GTX_SCAN_LINES_ON_DEVICE", "GTX_LINES_TIMING")}
    verdict = []
    for min_reads in ("10", "0"):
        args = ["counts", "-g", genome, "-w", str(SIZE), "-d", str(STEP), "-min", min_reads, reads]
        for to_pipe in (False, True):
            times = {name: [] for name, _ in tools}
            for r in range(runs):
                for name, tool in tools:
                    dt, rss, rc, nbytes, md5 = run_tool(tool, args, to_pipe, out, env, r == 0)
                    times[name].append(dt)
                    print("e2e -min %-2s to a %s run %d %-9s %.2f s, peak host memory %.2f GB (rc %d, %d bytes of stdout%s)"
                          % (min_reads, "pipe" if to_pipe else "file", r, name, dt, rss, rc, nbytes, "" if md5 is None else ", md5 " + md5), flush=True)
            shape = "-min %s to a %s" % (min_reads, "pipe" if to_pipe else "file")
            for name, _ in tools:
                t = sorted(times[name])
                print("e2e %s: %-9s median %.2f s, range %.2f .. %.2f s" % (shape, name, t[len(t) // 2], t[0], t[-1]), flush=True)
            if parent:
                a, b = sorted(times["this tree"]), sorted(times["parent"])
                bound = b[len(b) // 2] + (b[-1] - b[0])
                verdict.append((shape, a[len(a) // 2], bound))
        timing = dict(env, GTX_LINES_TIMING="1")
        pr = subprocess.run([tools[0][1]] + args, stdout=open(out, "wb"), stderr=subprocess.PIPE, env=timing)
        print("e2e -min %s to a file, GTX_LINES_TIMING=1: %s" % (min_reads, " ".join(l for l in pr.stderr.decode().splitlines() if "[gtx lines]" in l)), flush=True)
    for shape, med, bound in verdict:
        print("default rule, %s: this tree's median %.2f s against the parent's median plus its range %.2f s: %s" % (shape, med, bound, "holds" if med <= bound else "LOSES"), flush=True)
    for f in (out, reads, genome):
        os.remove(f)


n_win = int(flag_val("--windows") or 248_000_000)
if n_win > 0:
    part1(n_win)
n_e2e = int(flag_val("--e2e") or 10_000_000)
if n_e2e > 0:
    part2(n_e2e, int(flag_val("--runs") or 5), flag_val("--parent"))
