#!/usr/bin/env python3
"""The -r filter of `genomic_scans counts` on the device (gtx_window_refs / gtx_window_filter_device, csrc/gtx_filter.hip), measured on
one MI355X.

Part 1, the pass: synthetic window vectors resident in HBM (48 classes: 24 chromosomes x 2 strands, -w 500 -d 25) of 31 M, 124 M and
248 M windows; 1 M reference regions laid out in islands so that they cover about 1 %, 10 % and 90 % of the windows; min_value 0 and a
min_value that keeps about 0.1 % of all windows.  Per shape:
  * gtx_window_refs (copy, device sort, running maximum) once, by the host's clock;
  * the filter call (three launches and the 8-byte read-back of the count; median and minimum of REPS calls by the host's clock: the
    call returns when the result is complete), the bytes it has to move -- the tiles a region reaches read once by the count pass, the
    tiles that hold a kept window once more by the emit pass, 16 bytes per kept window, the tile counts and bases; the searches'
    reads of the region arrays are NOT counted -- and the rate that makes, as a fraction of the HBM peak bench.py's `roofline` uses;
  * beside it gtx_window_select_device without controls on the same vector with the critical count at min_value (the sibling pass:
    every window read, an ordinal and a 4-byte row per kept window), and the copy of the vector to page-locked host memory that the
    per-window host loop needs before it can start.
Part 2 (--e2e N, default 10 M reads; 0: skip), the tool: `genomic_scans counts -r REF -w 500 -d 25 -min 10`, strand-aware, on N BED
reads over a genome of human size, the device route, GTX_SCAN_FILTER_ON_DEVICE=0, and the device route again, by the wall clock, with the
md5 of both outputs; and the same run without -r, which is what either route adds its filter to.
Usage: bench_scan_filter.py [--windows N,N,..] [--refs M] [--e2e N] [--dir D]"""
import hashlib, os, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "ibm-cbc-genomic-tools_amd")); sys.path.insert(0, R)
flag_val = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
d = flag_val("--dir") or os.environ.get("TMPDIR", "/tmp")
REPS = 9
STEP, SIZE, N_CLASSES, ISLANDS = 25, 500, 48, 64
HBM_PEAK_GBS = 8000.0                                                     # bench.py's roofline peak
# human chromosomes 1..22, X, Y (GRCh38, rounded to kb): the genome of part 2
HUMAN = [248956, 242193, 198295, 190214, 181538, 170805, 159345, 145138, 138394, 133797, 135086, 133275, 114364, 107043, 101991, 90338, 83257,
         80373, 58617, 64444, 46709, 50818, 156040, 57227]


def regions(rng, m, frac, class_len, n):
    """m regions over the classes, inside ISLANDS islands per class that hold `frac` of its positions, long enough to fill them"""
    import numpy as np
    length = max(50, int(3.0 * frac * n * STEP / m) - SIZE)
    cls = rng.integers(0, N_CLASSES, size=m)
    pitch = class_len // ISLANDS
    start = rng.integers(0, ISLANDS, size=m) * pitch + (rng.random(m) * pitch * frac).astype(np.int64) + 1
    stop = np.minimum(start + rng.integers(length // 2, length + 1, size=m), class_len + 5000)
    return np.stack([cls, start, stop], axis=1).astype(np.int32)


def time_calls(fn):
    import torch
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], min(ts)


def part1():
    import numpy as np, torch, gtx
    dev = torch.device("cuda:0")
    e = gtx.Engine(0)
    sizes = [int(x) for x in (flag_val("--windows") or "31000000,124000000,248000000").split(",")]
    m = int(flag_val("--refs") or 1_000_000)
    tile = gtx.FILTER_TILE
    print("tile %d windows; %d regions; -w %d -d %d over %d classes; REPS %d" % (tile, m, SIZE, STEP, N_CLASSES, REPS), flush=True)
    for n_want in sizes:
        per = n_want // N_CLASSES
        n = per * N_CLASSES
        class_len = (per - 1) * STEP + SIZE
        cl = np.full(N_CLASSES, class_len, dtype=np.int32)
        off = np.arange(N_CLASSES, dtype=np.int64) * per
        g = torch.Generator(device=dev); g.manual_seed(7)
        v = torch.poisson(torch.full((n,), 3.0, device=dev), generator=g).to(torch.int64)       # counts as a scan leaves them, a few windows far above
        v = torch.where(torch.rand(n, device=dev, generator=g) < 0.002, v * 40, v)
        high = int(torch.quantile(v[:4_000_000].float(), 0.999).item()) + 1                        # about 0.1 % of all windows reach it
        pinned = torch.empty(n, dtype=torch.int64).pin_memory()
        tc = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter(); pinned.copy_(v, non_blocking=True); torch.cuda.synchronize(); tc.append((time.perf_counter() - t0) * 1e3)
        copy_ms = sorted(tc)[1]
        del pinned
        print("%d windows (%.2f GB): the vector to page-locked host memory %.1f ms (%.1f GB/s); values >= %d in %.3f %% of the windows"
              % (n, n * 8 / 1e9, copy_ms, n * 8 / copy_ms / 1e6, high, 100.0 * float((v >= high).float().mean().item())), flush=True)
        d_o = torch.empty(n, dtype=torch.int64, device=dev); d_v = torch.empty(n, dtype=torch.int64, device=dev); d_r = torch.empty(n, dtype=torch.int32, device=dev)
        tiles = (n + tile - 1) // tile
        for frac in (0.01, 0.1, 0.9):
            refs = regions(np.random.default_rng(int(frac * 100)), m, frac, class_len, n)
            t0 = time.perf_counter(); e.window_refs(refs, cl, off, STEP, SIZE); prep_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter(); e.window_refs(refs, cl, off, STEP, SIZE); prep_ms = min(prep_ms, (time.perf_counter() - t0) * 1e3)
            flt = lambda mv: e.window_filter(v.data_ptr(), mv, n_windows=n, capacity=n, device_out=(d_o.data_ptr(), d_v.data_ptr()))
            covered = flt(0)
            reached = int(torch.unique(d_o[:covered] // tile).numel())                              # the tiles a region reaches
            for mv in (0, high):
                kept = flt(mv)
                live = reached if mv == 0 else int(torch.unique(d_o[:kept] // tile).numel())
                med, lo = time_calls(lambda: flt(mv))
                moved = reached * tile * 8.0 + live * tile * 8.0 + kept * 16.0 + tiles * (4 + 4 + 8 + 16)
                sel = lambda: e.window_select([v.data_ptr()], [np.array([mv], dtype=np.int32)], 1 << 30, n_windows=n, capacity=n, device_out=(d_o.data_ptr(), d_r.data_ptr()))
                s_kept = sel()
                s_live = int(torch.unique(d_o[:s_kept] // tile).numel()) if mv else tiles
                s_med, s_lo = time_calls(sel)
                s_moved = n * 8.0 + s_live * tile * 8.0 + s_kept * 12.0 + tiles * (4 + 4 + 8 + 16)
                print("  regions over %.1f %% of the windows (%.1f %% of the tiles), min_value %d: %d kept (%.3f %%) | gtx_window_refs %.1f ms | "
                      "filter %.3f ms (min %.3f) for %.3f GB = %.0f GB/s = %.2f of the %.0f GB/s peak | select, no controls, same vector: %d kept, %.3f ms (min %.3f) "
                      "for %.3f GB = %.0f GB/s | filter / select = %.2f | copy to host alone / filter = %.0fx"
                      % (100.0 * covered / n, 100.0 * reached / tiles, mv, kept, 100.0 * kept / n, prep_ms, med, lo, moved / 1e9, moved / med / 1e6,
                         moved / med / 1e6 / HBM_PEAK_GBS, HBM_PEAK_GBS, s_kept, s_med, s_lo, s_moved / 1e9, s_moved / s_med / 1e6, med / s_med, copy_ms / med), flush=True)
        del v, d_o, d_v, d_r
        torch.cuda.empty_cache()
    e.close()


def part2(n_reads):
    import numpy as np
    rng = np.random.default_rng(11)
    names = ["chr%s" % x for x in list(range(1, 23)) + ["X", "Y"]]
    lengths = np.asarray(HUMAN, dtype=np.int64) * 1000
    genome, reads, refs = os.path.join(d, "scanfilter_genome.bed"), os.path.join(d, "scanfilter_reads.bed"), os.path.join(d, "scanfilter_refs.bed")
    with open(genome, "w") as f:
        f.write("".join("%s\t0\t%d\n" % (nm, ln) for nm, ln in zip(names, lengths)))
    p = lengths / lengths.sum()
    def bed(path, n, span, clustered):
        c = rng.choice(len(names), size=n, p=p)
        s = (rng.random(n) * (lengths[c] - span - 1)).astype(np.int64)
        if clustered:                                                      # half of the reads in 5000 peaks of 2 kb
            pk = rng.integers(0, n, size=5000)
            k = rng.integers(0, 5000, size=n // 2)
            c[:n // 2] = c[pk][k]; s[:n // 2] = np.maximum(s[pk][k] + rng.integers(-1000, 1000, size=n // 2), 0)
        e = s + span
        m = rng.integers(0, 2, size=n)
        with open(path, "w") as f:
            for lo in range(0, n, 1 << 20):
                hi = min(n, lo + (1 << 20))
                f.write("".join("%s\t%d\t%d\tr\t0\t%s\n" % (names[a], b, x, "+-"[y]) for a, b, x, y in zip(c[lo:hi].tolist(), s[lo:hi].tolist(), e[lo:hi].tolist(), m[lo:hi].tolist())))
    t0 = time.perf_counter(); bed(reads, n_reads, 36, True); bed(refs, 20000, 2000, False)
    print("e2e: %d reads and 20000 reference regions written in %.1f s" % (n_reads, time.perf_counter() - t0), flush=True)
    tool = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_scans")
    base = [tool, "counts", "-g", genome, "-w", str(SIZE), "-d", str(STEP), "-min", "10"]
    out = os.path.join(d, "scanfilter.out")
    runs = [("no -r (PrintRemaining)", base + [reads], None), ("-r, filter on the device", base + ["-r", refs, reads], None),
            ("-r, GTX_SCAN_FILTER_ON_DEVICE=0", base + ["-r", refs, reads], "0"), ("-r, filter on the device", base + ["-r", refs, reads], None)]
    for name, cmd, env in runs:
        ev = dict(os.environ)
        ev.pop("GTX_SCAN_FILTER_ON_DEVICE", None)
        if env is not None:
            ev["GTX_SCAN_FILTER_ON_DEVICE"] = env
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=open(out, "wb"), stderr=subprocess.PIPE, env=ev)
        dt = time.perf_counter() - t0
        data = open(out, "rb").read()
        print("e2e %-34s %.2f s (rc %d, %d lines, md5 of stdout %s)" % (name, dt, r.returncode, data.count(b"\n"), hashlib.md5(data).hexdigest()[:12]), flush=True)


if (flag_val("--windows") or "x") != "0":
    part1()
n_e2e = int(flag_val("--e2e") or 10_000_000)
if n_e2e > 0:
    part2(n_e2e)
