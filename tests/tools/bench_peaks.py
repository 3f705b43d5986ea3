#!/usr/bin/env python3
"""The candidate selection of `genomic_scans peaks` on the device (gtx_peak_select_device, csrc/gtx_peaks.hip), measured on one MI355X.

Part 1, the pass: synthetic window vectors resident in HBM (Poisson counts of mean 3, as a scan leaves them; -w 500) of --windows
windows (default 248 M: a human-size genome at -w 500 -d 25, one strand), a min_reads that keeps about 50 %, 1 % and 0.001 % of them,
without and with a mappability vector.  Per shape the call (three launches and the 8-byte read-back of the count; median and minimum of
REPS calls by the host's clock: the call returns when the result is complete), its algorithmic bytes -- 16 B per window read, 24 B with
the mappability vector, 32 B per kept window written; the second read of the tiles that keep a window is NOT counted -- and the rate that
makes, as a fraction of the HBM peak bench.py's `roofline` uses.  Beside it gtx_window_select_device without controls on the signal
vector with the critical count at min_reads (the sibling pass: 8 B per window read, 12 B per kept window written).
Part 2 (--e2e N, default 10 M signal and 10 M control reads; 0: skip), the tool: `genomic_scans peaks -g GENOME -w 500 -d 25` over a
genome of human size, strand-aware and -i, RUNS times each with the selection on the device and with GTX_PEAKS_ON_DEVICE=0 (the
per-window loop on the host), alternating: wall time and peak resident host memory of the process (wait4), the md5 of stdout.
Usage: bench_peaks.py [--windows N] [--e2e N] [--runs K] [--dir D]"""
import hashlib, os, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(R, "ibm-cbc-genomic-tools_amd")); sys.path.insert(0, R)
flag_val = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
d = flag_val("--dir") or os.environ.get("TMPDIR", "/tmp")
REPS = 9
HBM_PEAK_GBS = 8000.0                                                     # bench.py's roofline peak
# human chromosomes 1..22, X, Y (GRCh38, rounded to kb): the genome of part 2
HUMAN = [248956, 242193, 198295, 190214, 181538, 170805, 159345, 145138, 138394, 133797, 135086, 133275, 114364, 107043, 101991, 90338, 83257,
         80373, 58617, 64444, 46709, 50818, 156040, 57227]


def time_calls(fn):
    import torch
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], min(ts)


def part1(n):
    import numpy as np, torch, gtx
    dev = torch.device("cuda:0")
    e = gtx.Engine(0)
    g = torch.Generator(device=dev); g.manual_seed(7)
    S = torch.poisson(torch.full((n,), 3.0, device=dev), generator=g).to(torch.int64)
    C = torch.poisson(torch.full((n,), 3.0, device=dev), generator=g).to(torch.int64)
    U = torch.randint(400, 501, (n,), device=dev, generator=g, dtype=torch.int64)            # (clamps nothing: the same windows are kept)
    print("%d windows (%.2f GB per vector), tile %d, REPS %d" % (n, n * 8 / 1e9, gtx.PEAK_TILE, REPS), flush=True)
    for min_reads in (3, 8, 13):
        cap = int((S >= min_reads).sum().item()) + 1
        d_o = torch.empty(cap, dtype=torch.int64, device=dev); d_r = torch.empty(3 * cap, dtype=torch.int64, device=dev); d_r32 = torch.empty(cap, dtype=torch.int32, device=dev)
        sel = lambda: e.window_select([S.data_ptr()], [np.array([min_reads], dtype=np.int32)], 1 << 30, n_windows=n, capacity=cap, device_out=(d_o.data_ptr(), d_r32.data_ptr()))
        s_kept = sel()
        s_med, s_lo = time_calls(sel)
        s_bytes = n * 8.0 + s_kept * 12.0
        for uniq in (None, U):
            for norm, ratio in ((False, 1.0), (True, 0.8)):
                call = lambda: e.peak_select_device(S.data_ptr(), C.data_ptr(), 500, min_reads, cap, d_o.data_ptr(), d_r.data_ptr(), uniq=None if uniq is None else uniq.data_ptr(),
                                                    norm=norm, p_ratio=ratio, n_windows=n)
                kept = call()
                assert kept == cap - 1 and kept == s_kept
                med, lo = time_calls(call)
                moved = n * (16.0 if uniq is None else 24.0) + kept * 32.0
                print("  min_reads %2d%s%s: %d kept (%.4f %%) | peak select %.3f ms (min %.3f) for %.3f GB = %.0f GB/s = %.2f of the %.0f GB/s peak | "
                      "gtx_window_select, no controls, signal vector: %.3f ms (min %.3f) for %.3f GB = %.0f GB/s | peak / select = %.2f"
                      % (min_reads, ", with U" if uniq is not None else ", no U  ", ", -norm 0.8" if norm else "          ", kept, 100.0 * kept / n, med, lo, moved / 1e9,
                         moved / med / 1e6, moved / med / 1e6 / HBM_PEAK_GBS, HBM_PEAK_GBS, s_med, s_lo, s_bytes / 1e9, s_bytes / s_med / 1e6, med / s_med), flush=True)
        del d_o, d_r, d_r32
    e.close()


def part2(n_reads, runs):
    import numpy as np
    rng = np.random.default_rng(11)
    names = ["chr%s" % x for x in list(range(1, 23)) + ["X", "Y"]]
    lengths = np.asarray(HUMAN, dtype=np.int64) * 1000
    genome, signal, control = os.path.join(d, "peaks_genome.bed"), os.path.join(d, "peaks_signal.bed"), os.path.join(d, "peaks_control.bed")
    with open(genome, "w") as f:
        f.write("".join("%s\t0\t%d\n" % (nm, ln) for nm, ln in zip(names, lengths)))
    p = lengths / lengths.sum()
    def bed(path, n, clustered):
        c = rng.choice(len(names), size=n, p=p)
        s = (rng.random(n) * (lengths[c] - 37)).astype(np.int64)
        if clustered:                                                      # half of the reads in 5000 peaks of 2 kb
            pk = rng.integers(0, n, size=5000)
            k = rng.integers(0, 5000, size=n // 2)
            c[:n // 2] = c[pk][k]; s[:n // 2] = np.maximum(s[pk][k] + rng.integers(-1000, 1000, size=n // 2), 0)
        m = rng.integers(0, 2, size=n)
        with open(path, "w") as f:
            for lo in range(0, n, 1 << 20):
                hi = min(n, lo + (1 << 20))
                f.write("".join("%s\t%d\t%d\tr\t0\t%s\n" % (names[a], b, b + 36, "+-"[y]) for a, b, y in zip(c[lo:hi].tolist(), s[lo:hi].tolist(), m[lo:hi].tolist())))
    t0 = time.perf_counter(); bed(signal, n_reads, True); bed(control, n_reads, False)
    print("e2e: %d signal and %d control reads written in %.1f s" % (n_reads, n_reads, time.perf_counter() - t0), flush=True)
    tool = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_scans")
    out = os.path.join(d, "peaks.out")
    for mode, flags in (("strand-aware", []), ("-i", ["-i"])):
        cmd = [tool, "peaks"] + flags + ["-g", genome, "-w", "500", "-d", "25", signal, control]
        for k in range(runs):
            for name, env in (("selection on the device", None), ("GTX_PEAKS_ON_DEVICE=0", "0")):
                ev = dict(os.environ)
                ev.pop("GTX_PEAKS_ON_DEVICE", None)
                if env is not None:
                    ev["GTX_PEAKS_ON_DEVICE"] = env
                t0 = time.perf_counter()
                pr = subprocess.Popen(cmd, stdout=open(out, "wb"), stderr=subprocess.DEVNULL, env=ev)
                _, status, ru = os.wait4(pr.pid, 0)
                dt = time.perf_counter() - t0
                data = open(out, "rb").read()
                print("e2e %-12s run %d %-24s %.2f s, peak host memory %.2f GB (rc %d, %d lines, md5 of stdout %s)"
                      % (mode, k, name, dt, ru.ru_maxrss / 1e6, os.waitstatus_to_exitcode(status), data.count(b"\n"), hashlib.md5(data).hexdigest()[:12]), flush=True)


n_win = int(flag_val("--windows") or 248_000_000)
if n_win > 0:
    part1(n_win)
n_e2e = int(flag_val("--e2e") or 10_000_000)
if n_e2e > 0:
    part2(n_e2e, int(flag_val("--runs") or 3))
