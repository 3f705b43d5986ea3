#!/usr/bin/env python3
"""Link (gtx_link_device, genomic_regions link), measured on one MI355X.

1. gtx_link_device on HBM-resident reads in (class, start) order -- bench.py's workload: reads of 50 bp on 24 classes, which at 100 M
   reads cover the genome 1.6 times over and link into few, large groups under -d 1000 -- then the same number of reads of 2 bp (thin:
   most groups are singletons), each without a fold and with GTX_LINK_SUM.  Beside every figure, from the same process on the same
   box: one `count` step (gtx_count_device) on the same reads and the bare load pattern (scripts/membench.hip, its best x3 line) --
   the ceilings a reader of 12 B per read is judged against -- and the one-core host walk of the same packed triples
   (tests/tools/link_walk.c) -- the floor the device path has to beat to be worth having.  Results are compared with the walk's first.
2. `genomic_regions link` end to end from a BED file, without a label function and with --label-func sum.
Usage: bench_link.py [n_reads] [n_refs] [n_reads_cli] [--dir D] [--passes-only | --cli-only]"""
import ctypes, os, re, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
BIN = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc")
flag_val = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
skip = {sys.argv.index(f) + 1 for f in ("--dir",) if f in sys.argv}
args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 100_000_000
m = int(args[1]) if len(args) > 1 else 1_000_000
n_cli = int(args[2]) if len(args) > 2 else 20_000_000
d = flag_val("--dir") or os.environ.get("TMPDIR", "/tmp")
REPS = 15


def host_walk():
    so = os.path.join(d, "liblink_walk.so")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(R, "tests", "tools", "link_walk.c")], check=True)
    f = ctypes.CDLL(so).link_walk
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int64] * 2 + [ctypes.c_void_p] * 5
    return f


def bare_load():
    """GB/s of the best x3 non-temporal line of scripts/membench.hip at n reads (None: not built and no hipcc)"""
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


def passes():
    import numpy as np
    import torch
    import gtx
    from gtx import synth
    dev = torch.device("cuda:0")
    walk = host_walk()
    e = gtx.Engine(0)
    e.set_refs(synth.genome_intervals(m, 43, 50, 2000), synth.n_classes())

    def reads_on_device(length):
        per = synth.apportion(n, synth.CHROM_LEN)
        out = torch.empty((n, 3), dtype=torch.int32, device=dev)
        at = 0
        for ci, cnt in enumerate(per):
            cnt = int(cnt)
            g = torch.Generator(device=dev); g.manual_seed(44000 + ci)
            s, _ = torch.sort(torch.randint(1, int(synth.CHROM_LEN[ci]) - 51, (cnt,), device=dev, generator=g, dtype=torch.int32))
            out[at:at + cnt, 0] = ci; out[at:at + cnt, 1] = s; out[at:at + cnt, 2] = s + length - 1
            at += cnt
        return out

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); f(); e.sync()
        return (time.perf_counter() - t0) * 1e3

    gbs = bare_load()
    bare_ms = None if gbs is None else 12.0 * n / gbs / 1e6
    print("bare load pattern at %d reads: %s" % (n, "not measured" if gbs is None else "%.0f GB/s = %.3f ms for 12 B per read" % (gbs, bare_ms)), flush=True)
    g = torch.Generator(device=dev); g.manual_seed(5)
    vals = torch.randint(0, 1000, (n,), device=dev, generator=g, dtype=torch.int64)
    h_vals = vals.cpu().numpy()
    for name, length, dist in (("50 bp, -d 0", 50, 0), ("50 bp, -d 1000 (few large groups)", 50, 1000), ("2 bp, -d 0 (mostly singletons)", 2, 0)):
        reads = reads_on_device(length)
        h_reads = reads.cpu().numpy()
        head = torch.zeros(n, dtype=torch.int32, device=dev); cnt = torch.zeros_like(head); stop = torch.zeros_like(head)
        fold = torch.zeros(n, dtype=torch.int64, device=dev)
        hits = torch.zeros(m, dtype=torch.int64, device=dev)
        info = [None]

        def f_link():
            info[0] = e.link_device(reads.data_ptr(), n, head.data_ptr(), cnt.data_ptr(), stop.data_ptr(), None, None, dist, 0)

        def f_sum():
            info[0] = e.link_device(reads.data_ptr(), n, head.data_ptr(), cnt.data_ptr(), stop.data_ptr(), vals.data_ptr(), fold.data_ptr(), dist, gtx.LINK_SUM)
        f_count = lambda: e.count_device(reads.data_ptr(), n, hits.data_ptr(), None, gtx.READS_SORTED)
        for f in (f_link, f_sum, f_count):
            timed(f)
        # the host walk, once with the sum: the device's answer is held to it
        wh, wc, ws = (np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32))
        wv = np.zeros(n, dtype=np.int64); wu = ctypes.c_int64(0)
        t0 = time.perf_counter()
        groups = walk(h_reads.ctypes.data, h_vals.ctypes.data, n, dist, wh.ctypes.data, wc.ctypes.data, ws.ctypes.data, wv.ctypes.data, ctypes.byref(wu))
        walk_sum_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        walk(h_reads.ctypes.data, None, n, dist, wh.ctypes.data, wc.ctypes.data, ws.ctypes.data, None, ctypes.byref(wu))
        walk_ms = (time.perf_counter() - t0) * 1e3
        timed(f_sum)
        same = (info[0].n_groups == groups and info[0].first_unsorted == wu.value == -1
                and np.array_equal(head[:groups].cpu().numpy().view(np.uint32), wh[:groups]) and np.array_equal(cnt[:groups].cpu().numpy().view(np.uint32), wc[:groups])
                and np.array_equal(stop[:groups].cpu().numpy(), ws[:groups]) and np.array_equal(fold[:groups].cpu().numpy(), wv[:groups]))
        t = {"link": [], "sum": [], "count": []}
        for _ in range(REPS):                                                # alternating: the three see the same machine
            t["link"].append(timed(f_link)); t["sum"].append(timed(f_sum)); t["count"].append(timed(f_count))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        lo = {k: min(v) for k, v in t.items()}
        print("%-36s %d reads -> %d groups (%.1f %% singletons): link %.3f ms (min %.3f) | with GTX_LINK_SUM %.3f ms (min %.3f) | count step %.3f ms (min %.3f) | "
              "bare load %s | host walk, one core %.1f ms (with the sum %.1f ms) | link / count = %.2fx, link / bare load = %s, host walk / link = %.0fx | "
              "%.0f GB/s of 12 B per read | device == host walk: %s"
              % (name, n, groups, 100.0 * float((wc[:groups] == 1).mean()) if groups else 0.0, med["link"], lo["link"], med["sum"], lo["sum"], med["count"], lo["count"],
                 "n/a" if bare_ms is None else "%.3f ms" % bare_ms, walk_ms, walk_sum_ms, med["link"] / med["count"],
                 "n/a" if bare_ms is None else "%.2fx" % (med["link"] / bare_ms), walk_ms / med["link"], 12.0 * n / med["link"] / 1e6, same), flush=True)
        if not same:
            sys.exit("the device and the host walk disagree")
        del reads, head, cnt, stop, fold, hits
    e.close()


def cli():
    pack, tool = os.path.join(BIN, "gtx_packtool"), os.path.join(BIN, "genomic_regions")
    bed, out = os.path.join(d, "blink_reads_%d.bed" % n_cli), os.path.join(d, "blink_out")
    subprocess.run([pack, "synth", str(n_cli), "44", bed, "50"], check=True)
    print("reads: %d lines, %.3f GB; cores available: %d" % (n_cli, os.path.getsize(bed) / 1e9, len(os.sched_getaffinity(0))), flush=True)

    def once(cmd):
        t0 = time.perf_counter()
        try:
            with open(out, "wb") as f:
                r = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, env=dict(os.environ, GTX_TEXT_TRACE="1"), timeout=600)
        except subprocess.TimeoutExpired:
            sys.exit("timed out: %s" % " ".join(cmd))                       # (a GPU step that hangs or fails ends the run: nothing more is started)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            sys.exit("failed (rc %d): %s" % (r.returncode, r.stderr.decode()[-2000:]))
        return dt, " ".join(l for l in r.stderr.decode().splitlines() if l.startswith("[gtx text]"))

    for label, cmd in (("link", [tool, "link", bed]), ("link -d 1000", [tool, "link", "-d", "1000", bed]), ("link --label-func sum", [tool, "link", "--label-func", "sum", bed])):
        once(cmd)                                                            # (page cache warm, first-run costs out)
        ts = []
        for _ in range(3):
            dt, tr = once(cmd)
            ts.append(dt)
        print("%-24s %.3f s (median of 3; runs %s), %.1f M lines/s, %.3f GB written  %s"
              % (label, sorted(ts)[1], " ".join("%.3f" % x for x in ts), n_cli / sorted(ts)[1] / 1e6, os.path.getsize(out) / 1e9, tr), flush=True)
    for p in (bed, out):
        os.remove(p)


if "--cli-only" not in sys.argv:
    passes()
if "--passes-only" not in sys.argv:
    cli()
