#!/usr/bin/env python3
"""The neighbour passes (gtx_adjacent_device, gtx_gaps_device), measured on one MI355X.

Regions resident in HBM in (class, start) order -- bench.py's workload: 24 classes, region starts uniform over the chromosomes -- at
three lengths, which at 100 M regions give three gap densities: 1000 bp (hardly a gap), 50 bp (a gap behind every fifth region), 2 bp
(a gap behind nearly every region).  Per length: gtx_adjacent_device without and with distances, gtx_gaps_device, and beside them,
from the same process on the same box, gtx_link_device (-d 0, no fold: three passes over the same triples), one `count` step
(gtx_count_device, bench.py's streaming kernel) and the bare load pattern (scripts/membench.hip, its best x3 line) -- the ceilings a
reader of 12 B per region is judged against -- and the one-core host walks of the same packed triples (tests/tools/adjacent_walk.c),
the floor the device path has to beat to be worth having.  Results are compared with the walks' first.  Warm-up calls first, then
REPS alternating repetitions; medians with the minimum and maximum beside them.
Usage: bench_adjacent.py [n_regions] [n_refs] [--dir D]"""
import ctypes, os, re, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
flag_val = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
skip = {sys.argv.index(f) + 1 for f in ("--dir",) if f in sys.argv}
args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 100_000_000
m = int(args[1]) if len(args) > 1 else 1_000_000
d = flag_val("--dir") or os.environ.get("TMPDIR", "/tmp")
REPS = 15


def host_walks():
    so = os.path.join(d, "libadjacent_walk.so")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(R, "tests", "tools", "adjacent_walk.c")], check=True)
    lib = ctypes.CDLL(so)
    lib.adjacent_walk.restype = None
    lib.adjacent_walk.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.gaps_walk.restype = ctypes.c_int64
    lib.gaps_walk.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 4
    return lib


def bare_load():
    """GB/s of the best x3 non-temporal line of scripts/membench.hip at n regions (None: not built and no hipcc)"""
    exe = os.path.join(R, "scripts", "membench.bin")
    if not os.path.exists(exe):
        if subprocess.run(["hipcc", "-O3", "--offload-arch=gfx950", "-o", exe, os.path.join(R, "scripts", "membench.hip")]).returncode != 0:
            return None
    try:
        out = subprocess.run([exe, str(n)], capture_output=True, timeout=300).stdout.decode()
    except subprocess.TimeoutExpired:
        sys.exit("membench timed out")
    rates = [float(x) for x in re.findall(r"^x3 depth4-nt .* (\d+) GB/s$", out, re.M)]
    return max(rates) if rates else None


def main():
    import numpy as np
    import torch
    import gtx
    from gtx import synth
    dev = torch.device("cuda:0")
    walks = host_walks()
    e = gtx.Engine(0)
    e.set_refs(synth.genome_intervals(m, 43, 50, 2000), synth.n_classes())
    bounds = np.asarray(synth.CHROM_LEN, dtype=np.int64)

    def regions_on_device(length):
        per = synth.apportion(n, synth.CHROM_LEN)
        out = torch.empty((n, 3), dtype=torch.int32, device=dev)
        at = 0
        for ci, cnt in enumerate(per):
            cnt = int(cnt)
            g = torch.Generator(device=dev); g.manual_seed(44000 + ci)
            s, _ = torch.sort(torch.randint(1, int(synth.CHROM_LEN[ci]) - 1001, (cnt,), device=dev, generator=g, dtype=torch.int32))
            out[at:at + cnt, 0] = ci; out[at:at + cnt, 1] = s; out[at:at + cnt, 2] = s + length - 1
            at += cnt
        return out

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); f(); e.sync()
        return (time.perf_counter() - t0) * 1e3

    gbs = bare_load()
    bare_ms = None if gbs is None else 12.0 * n / gbs / 1e6
    print("bare load pattern at %d regions: %s" % (n, "not measured" if gbs is None else "%.0f GB/s = %.3f ms for 12 B per region" % (gbs, bare_ms)), flush=True)
    g = torch.Generator(device=dev); g.manual_seed(5)
    minus = torch.randint(0, 2, (n,), device=dev, generator=g, dtype=torch.uint8)
    h_minus = minus.cpu().numpy()
    for name, length in (("1000 bp (hardly a gap)", 1000), ("50 bp", 50), ("2 bp (a gap nearly everywhere)", 2)):
        tri = regions_on_device(length)
        h_tri = tri.cpu().numpy()
        # the host walks first: the gaps needed, and what the device's answers are held to
        w_dist = np.zeros(n, dtype=np.int64); w_info = np.zeros(3, dtype=np.int64)
        t0 = time.perf_counter()
        walks.adjacent_walk(h_tri.ctypes.data, None, n, 0, 0, None, w_info.ctypes.data)
        walk_pair_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        walks.adjacent_walk(h_tri.ctypes.data, h_minus.ctypes.data, n, 2, 3, w_dist.ctypes.data, w_info.ctypes.data)
        walk_dist_ms = (time.perf_counter() - t0) * 1e3
        wo, ws, we = np.zeros(2 * n, dtype=np.uint32), np.zeros(2 * n, dtype=np.int32), np.zeros(2 * n, dtype=np.int32)
        g_info = np.zeros(2, dtype=np.int64)
        walks.gaps_walk(h_tri.ctypes.data, n, bounds.ctypes.data, len(bounds), wo.ctypes.data, ws.ctypes.data, we.ctypes.data, g_info.ctypes.data)   # (pages touched)
        t0 = time.perf_counter()
        n_gaps = walks.gaps_walk(h_tri.ctypes.data, n, bounds.ctypes.data, len(bounds), wo.ctypes.data, ws.ctypes.data, we.ctypes.data, g_info.ctypes.data)
        walk_gaps_ms = (time.perf_counter() - t0) * 1e3
        dist = torch.zeros(n, dtype=torch.int64, device=dev)
        owner = torch.zeros(max(n_gaps, 1), dtype=torch.int32, device=dev); gs = torch.zeros_like(owner); ge = torch.zeros_like(owner)
        head = torch.zeros(n, dtype=torch.int32, device=dev); cnt = torch.zeros_like(head); stop = torch.zeros_like(head)
        hits = torch.zeros(m, dtype=torch.int64, device=dev)
        info = {}

        def f_pair():
            info["pair"] = e.adjacent_device(tri.data_ptr(), n)

        def f_dist():
            info["dist"] = e.adjacent_device(tri.data_ptr(), n, minus.data_ptr(), 2, 3, dist.data_ptr())

        def f_gaps():
            info["gaps"] = e.gaps_device(tri.data_ptr(), n, bounds, n_gaps, owner.data_ptr(), gs.data_ptr(), ge.data_ptr())

        def f_link():
            info["link"] = e.link_device(tri.data_ptr(), n, head.data_ptr(), cnt.data_ptr(), stop.data_ptr(), None, None, 0, 0)
        f_count = lambda: e.count_device(tri.data_ptr(), n, hits.data_ptr(), None, gtx.READS_SORTED)
        fs = {"pair": f_pair, "dist": f_dist, "gaps": f_gaps, "link": f_link, "count": f_count}
        for f in fs.values():                                                # warm-up: first-call allocations and code loading are out
            timed(f); timed(f)
        want_pair = {"first_unsorted": int(w_info[0]), "n_inclusions": int(w_info[1]), "n_overlaps": int(w_info[2])}
        same = (info["pair"].as_dict() == want_pair and info["dist"].as_dict() == want_pair and np.array_equal(dist.cpu().numpy(), w_dist)
                and info["gaps"].as_dict() == {"n_gaps": n_gaps, "first_bad": int(g_info[0]), "bad_kind": int(g_info[1])} and g_info[0] == -1
                and np.array_equal(owner.cpu().numpy()[:n_gaps].view(np.uint32), wo[:n_gaps]) and np.array_equal(gs.cpu().numpy()[:n_gaps], ws[:n_gaps])
                and np.array_equal(ge.cpu().numpy()[:n_gaps], we[:n_gaps]))
        t = {k: [] for k in fs}
        for _ in range(REPS):                                                # alternating: all see the same machine
            for k, f in fs.items():
                t[k].append(timed(f))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        show = lambda k: "%.3f ms (min %.3f, max %.3f)" % (med[k], min(t[k]), max(t[k]))
        print("%-32s %d regions, %d inclusions, %d overlaps, %d gaps (%.2f per region)\n"
              "    adjacent (test)            %s = %.0f GB/s of 12 B per region\n"
              "    adjacent + distances       %s = %.0f GB/s of 21 B per region\n"
              "    gaps (inv)                 %s = %.0f GB/s of 24 B per region + 12 B per gap\n"
              "    link -d 0                  %s\n"
              "    count step                 %s\n"
              "    bare load                  %s\n"
              "    host walk, one core        pairs %.1f ms, with distances %.1f ms, gaps %.1f ms\n"
              "    adjacent / bare load = %s, adjacent / count = %.2fx, link / adjacent = %.2fx, gaps / adjacent = %.2fx, host walk / adjacent = %.0fx, host gaps / gaps = %.0fx\n"
              "    device == host walks: %s"
              % (name, n, w_info[1], w_info[2], n_gaps, n_gaps / n, show("pair"), 12.0 * n / med["pair"] / 1e6, show("dist"), 21.0 * n / med["dist"] / 1e6,
                 show("gaps"), (24.0 * n + 12.0 * n_gaps) / med["gaps"] / 1e6, show("link"), show("count"), "n/a" if bare_ms is None else "%.3f ms" % bare_ms,
                 walk_pair_ms, walk_dist_ms, walk_gaps_ms, "n/a" if bare_ms is None else "%.2fx" % (med["pair"] / bare_ms), med["pair"] / med["count"],
                 med["link"] / med["pair"], med["gaps"] / med["pair"], walk_pair_ms / med["pair"], walk_gaps_ms / med["gaps"], same), flush=True)
        if not same:
            sys.exit("the device and the host walks disagree")
        del tri, dist, owner, gs, ge, head, cnt, stop, hits
    e.close()


main()
