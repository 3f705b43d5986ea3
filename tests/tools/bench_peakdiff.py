#!/usr/bin/env python3
"""The window selection of genomic_peakdiff (gtx_window_select_device, csrc/gtx_select.hip), measured on one MI355X against what it
replaces.

Synthetic window vectors in HBM at the reference's defaults (-w 500 -d 100: 31 M windows per strand of a human genome, 62 M with both
strands), 4 vectors (2 + 2 replicates) and 8 (with controls), thresholds placed for about 0.1 %, 1 % and 50 % of the windows kept.
Per shape:
  * the select call (three launches and the 8-byte read-back of the count; median and minimum of REPS calls), its bytes -- every
    vector read by the count pass and, in the tiles that hold a kept window, once more by the emit pass, plus the kept windows'
    ordinals and rows -- and the rate that makes, as a
    fraction of the HBM peak bench.py's `roofline` uses and, with --bench-line FILE (a line bench.py printed on the same box), of the
    rate its streaming kernel achieved there;
  * today's alternative: hipMemcpy of all vectors to page-locked host memory, then the table rule in a one-core host loop
    (tests/tools/select_walk.c), whose result the device's is compared with.
The split of the call into its three kernels comes from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python
bench_peakdiff.py --shapes 1), not from here.
Usage: bench_peakdiff.py [--shapes K] [--bench-line FILE] [--dir D]"""
import ctypes, json, os, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
flag_val = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
d = flag_val("--dir") or os.environ.get("TMPDIR", "/tmp")
REPS = 9
W = 500
HBM_PEAK_GBS = 8000.0                                                     # bench.py's roofline peak


def host_walk():
    so = os.path.join(d, "libselect_walk.so")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(R, "tests", "tools", "select_walk.c")], check=True)
    f = ctypes.CDLL(so).select_walk
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return f


def main():
    import numpy as np
    import torch
    import gtx
    dev = torch.device("cuda:0")
    walk = host_walk()
    e = gtx.Engine(0)
    ceiling = None
    if flag_val("--bench-line"):
        line = [l for l in open(flag_val("--bench-line")) if l.startswith("{")][-1]
        ceiling = float(json.loads(line)["roofline"]["achieved"])
    shapes = [(n, nv, frac) for n in (31_000_000, 62_000_000) for nv in (4, 8) for frac in (0.001, 0.01, 0.5)]
    shapes = shapes[:int(flag_val("--shapes") or len(shapes))]
    tile, lds_max_w = gtx.window_select_limits()
    print("tile %d windows, tables in LDS up to W = %d; W = %d; bench.py streaming kernel on this box: %s" %
          (tile, lds_max_w, W, "not given" if ceiling is None else "%.0f GB/s" % ceiling), flush=True)
    pinned, vecs, shape_of = None, None, None
    for n, nv, frac in shapes:
        nt, ctl = (4, False) if nv == 4 else (4, True)
        if shape_of != (n, nv):
            # counts as a scan leaves them: Poisson-like around 3 per window, a few windows far above (the peaks)
            del vecs
            vecs = []
            for f in range(nv):
                g = torch.Generator(device=dev); g.manual_seed(100 + f)
                v = torch.poisson(torch.full((n,), 3.0, device=dev), generator=g).to(torch.int64)
                peak = torch.rand(n, device=dev, generator=g) < 0.002
                v = torch.where(peak, v * 40, v)
                vecs.append(v)
            if pinned is None or pinned.numel() < nv * n:
                pinned = torch.empty(nv * n, dtype=torch.int64).pin_memory()
            shape_of = (n, nv)
        # tables: a flat critical count per tested vector, chosen on vector 0's distribution so that all four together keep ~frac
        q = 1.0 - (1.0 - frac) ** (1.0 / nt)
        sample = vecs[0][:4_000_000].clamp(max=W).float()
        crit = int(torch.quantile(sample[:1_000_000], 1.0 - q).item()) + 1 if frac < 0.5 else int(torch.quantile(sample[:1_000_000], 1.0 - q).item())
        tables = [np.full(W + 1 if ctl else 1, crit, dtype=np.int32) for _ in range(nt)]
        tested = [v.data_ptr() for v in vecs[:nt]]
        controls = [v.data_ptr() for v in vecs[nt:]] if ctl else None
        cap = n if frac >= 0.5 else n // 8
        cols = nv
        d_o = torch.empty(cap, dtype=torch.int64, device=dev); d_r = torch.empty(cap * cols, dtype=torch.int32, device=dev)
        sel = lambda: e.window_select(tested, tables, W, controls=controls, n_windows=n, capacity=cap, device_out=(d_o.data_ptr(), d_r.data_ptr()))
        kept = sel()
        if kept > cap:
            sys.exit("capacity %d too small for %d kept" % (cap, kept))
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize(); t0 = time.perf_counter(); sel(); ts.append((time.perf_counter() - t0) * 1e3)
        med, lo = sorted(ts)[len(ts) // 2], min(ts)
        # bytes: the count pass reads every vector; the emit pass reads the tiles that hold a kept window (it leaves the others after
        # one look at their base) and writes an ordinal and a row per kept window; the tile counts and bases go through the prefix
        tiles = (n + tile - 1) // tile
        live = int(torch.unique(d_o[:kept] // tile).numel())
        bytes_moved = nv * n * 8.0 + live * tile * nv * 8.0 + kept * (8 + 4 * cols) + tiles * (4 + 4 + 8 + 16)
        rate = bytes_moved / med / 1e6
        # today's alternative: all vectors to page-locked memory, one host loop
        tc = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for f, v in enumerate(vecs):
                pinned[f * n:(f + 1) * n].copy_(v, non_blocking=True)
            torch.cuda.synchronize(); tc.append((time.perf_counter() - t0) * 1e3)
        copy_ms = sorted(tc)[1]
        h = pinned.numpy().view(np.uint64)
        hp = (ctypes.c_void_p * nv)(*[h[f * n:].ctypes.data for f in range(nv)])
        ht = (ctypes.c_void_p * nt)(*[t.ctypes.data for t in tables])
        wo, wr = np.empty(cap, dtype=np.int64), np.empty(cap * cols, dtype=np.int32)
        t0 = time.perf_counter()
        wk = walk(ctypes.addressof(hp), ctypes.addressof(hp) + 8 * nt if ctl else None, nt, n, W, ctypes.addressof(ht), wo.ctypes.data, wr.ctypes.data)
        walk_ms = (time.perf_counter() - t0) * 1e3
        same = wk == kept and np.array_equal(d_o[:kept].cpu().numpy(), wo[:kept]) and np.array_equal(d_r[:kept * cols].cpu().numpy(), wr[:kept * cols])
        print("%d windows x %d vectors, %.3f %% kept (%d, in %.0f %% of the tiles): select %.3f ms (min %.3f) = %.0f GB/s of %.2f GB moved = %.2f of the %.0f GB/s peak%s | "
              "copy to page-locked memory %.1f ms (%.1f GB/s) + one-core host loop %.1f ms = %.1f ms | alternative / select = %.0fx, copy alone / select = %.1fx | "
              "device == host loop: %s"
              % (n, nv, 100.0 * kept / n, kept, 100.0 * live / tiles, med, lo, rate, bytes_moved / 1e9, rate / HBM_PEAK_GBS, HBM_PEAK_GBS,
                 "" if ceiling is None else ", %.2f of bench.py's streaming kernel" % (rate / ceiling),
                 copy_ms, nv * n * 8 / copy_ms / 1e6, walk_ms, copy_ms + walk_ms, (copy_ms + walk_ms) / med, copy_ms / med, same), flush=True)
        if not same:
            sys.exit("the device and the host loop disagree")
        del d_o, d_r
    e.close()


main()
