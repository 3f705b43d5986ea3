#!/usr/bin/env python3
"""Per-query hits and genomic_subset, measured on one MI355X.

1. The hits pass alone (gtx_query_hits_device: the join's count walk and a narrowing pass) on HBM-resident reads against the count
   pass of the join as gtx_join_device makes it (no room for pairs: count walk, scan of the offsets, cut) and against one `count` step
   (gtx_count_device), the three alternating in one process: bench.py's workload (-i: sorted reads of 50 bp on 24 classes), the same
   reads shuffled, and strand-aware (48 classes alternating along a position-sorted stream).  Every call is timed by the host
   clock around a call that ends in a synchronise; results of the hits pass are compared with the join's offsets first.
2. `genomic_subset -S -i refs.bed reads.bed` end to end from a BED file: the text path (GTX_TEXT_ON_DEVICE=1) against the loop
   (=0) on the same file, outputs compared, and beside `genomic_overlaps count -S -i` on the same files.
With --trace, one run of each part under `rocprofv3 --kernel-trace --stats`: the kernels' own times.
Usage: bench_subset.py [n_reads] [n_refs] [n_reads_cli] [--big N [--big-loop]] [--trace] [--dir D] [--passes-only | --cli-only]
  --big N: the text path (and count) once more on a file of N reads; --big-loop: the loop there too, one run (about 4 M reads/s)"""
import csv, glob, os, shutil, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (R, os.path.join(R, "ibm-cbc-genomic-tools_amd")):
    sys.path.insert(0, p)
BIN = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc")
flag_val = lambda f: sys.argv[sys.argv.index(f) + 1] if f in sys.argv else None
skip = {sys.argv.index(f) + 1 for f in ("--dir", "--big") if f in sys.argv}                 # (the values of the two options that take one)
args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 100_000_000
m = int(args[1]) if len(args) > 1 else 1_000_000
n_cli = int(args[2]) if len(args) > 2 else 10_000_000
n_big = int(flag_val("--big") or 0)
d = flag_val("--dir") or os.environ.get("TMPDIR", "/tmp")
trace = "--trace" in sys.argv
REPS = 15


def passes():
    import numpy as np
    import torch
    import gtx
    from gtx import synth
    dev = torch.device("cuda:0")
    e = gtx.Engine(0)

    def reads_on_device(stranded, shuffled):
        per = synth.apportion(n, synth.CHROM_LEN)
        out = torch.empty((n, 3), dtype=torch.int32, device=dev)
        at = 0
        for ci, cnt in enumerate(per):
            cnt = int(cnt)
            g = torch.Generator(device=dev); g.manual_seed(44000 + ci)
            s, _ = torch.sort(torch.randint(1, int(synth.CHROM_LEN[ci]) - 51, (cnt,), device=dev, generator=g, dtype=torch.int32))
            out[at:at + cnt, 0] = ci
            if stranded:
                out[at:at + cnt, 0] += 24 * torch.randint(0, 2, (cnt,), device=dev, generator=g, dtype=torch.int32)
            out[at:at + cnt, 1] = s; out[at:at + cnt, 2] = s + 49
            at += cnt
        if shuffled:
            g = torch.Generator(device=dev); g.manual_seed(7)
            out = out[torch.randperm(n, device=dev, generator=g)].contiguous()
        return out

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); f(); e.sync()
        return (time.perf_counter() - t0) * 1e3

    for name, stranded, shuffled in (("sorted -i", False, False), ("shuffled -i", False, True), ("strand-aware", True, False)):
        refs = synth.genome_intervals(m, 43, 50, 2000, stranded=stranded)
        e.set_refs(refs, synth.n_classes(stranded))
        reads = reads_on_device(stranded, shuffled)
        hits = torch.zeros(n, dtype=torch.int32, device=dev)
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        cnt = torch.zeros(m, dtype=torch.int64, device=dev)
        flags = 0 if shuffled or stranded else gtx.READS_SORTED
        f_hits = lambda: e.query_hits_device(reads.data_ptr(), n, hits.data_ptr())
        f_join = lambda: e.join_device(reads.data_ptr(), n, off.data_ptr(), None, 0)
        f_count = lambda: e.count_device(reads.data_ptr(), n, cnt.data_ptr(), None, flags)
        for f in (f_hits, f_join, f_count):
            timed(f)                                                         # (code objects loaded, buffers made)
        total = e.join_device(reads.data_ptr(), n, off.data_ptr(), None, 0)[0]
        same = bool(torch.equal(hits.to(torch.int64), off[1:] - off[:-1]))
        share = float((hits > 0).float().mean())
        t = {"hits": [], "join": [], "count": []}
        for _ in range(REPS):                                                # alternating: the three see the same machine
            t["hits"].append(timed(f_hits)); t["join"].append(timed(f_join)); t["count"].append(timed(f_count))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        lo = {k: min(v) for k, v in t.items()}
        print("%-13s %d reads x %d regions: hits pass %.3f ms (min %.3f) | join count pass %.3f ms (min %.3f) | count step %.3f ms (min %.3f) | "
              "join / hits = %.2fx, hits / count = %.2fx | %.1f GB/s of 16 B per query | pairs %d, queries with a hit %.1f %%, hits == join offsets: %s"
              % (name, n, m, med["hits"], lo["hits"], med["join"], lo["join"], med["count"], lo["count"], med["join"] / med["hits"],
                 med["hits"] / med["count"], 16.0 * n / med["hits"] / 1e6, total, 100 * share, same), flush=True)
        if not same:
            sys.exit("the hits pass and the join disagree")
        del reads, hits, off, cnt
    e.close()


def cli():
    pack = os.path.join(BIN, "gtx_packtool")
    sub, ovl = os.path.join(BIN, "genomic_subset"), os.path.join(BIN, "genomic_overlaps")
    refs = os.path.join(d, "bsub_refs.bed")
    subprocess.run([pack, "synthrefs", str(m), "43", refs], check=True)

    def once(cmd, on_device, out_path):
        env = dict(os.environ, GTX_TEXT_ON_DEVICE=str(on_device), GTX_TEXT_TRACE="1")
        t0 = time.perf_counter()
        try:
            with open(out_path, "wb") as f:
                r = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, env=env, timeout=600)
        except subprocess.TimeoutExpired:
            sys.exit("timed out: %s" % " ".join(cmd))                       # (a GPU step that hangs or fails ends the run: nothing more is started)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            sys.exit("failed (rc %d): %s" % (r.returncode, r.stderr.decode()[-2000:]))
        tr = [l for l in r.stderr.decode().splitlines() if l.startswith("[gtx subset]") or l.startswith("[gtx text]")]
        return dt, tr[0] if tr else "(loop / host packer)"

    def series(label, cmd, on_device, out_path, reps=3):
        once(cmd, on_device, out_path)                                       # (page cache warm, first-run costs out)
        ts = []
        for _ in range(reps):
            dt, tr = once(cmd, on_device, out_path)
            ts.append(dt)
        print("%-34s %.3f s (median of %d; runs %s), %.3f GB written  %s" % (label, sorted(ts)[len(ts) // 2], reps, " ".join("%.3f" % x for x in ts),
                                                                          os.path.getsize(out_path) / 1e9, tr), flush=True)

    for nr, with_loop in ((n_cli, True),) + (((n_big, "--big-loop" in sys.argv),) if n_big else ()):
        bed = os.path.join(d, "bsub_reads_%d.bed" % nr)
        subprocess.run([pack, "synth", str(nr), "44", bed, "50"], check=True)
        print("reads: %d lines, %.3f GB; refs: %d lines; cores available: %d" % (nr, os.path.getsize(bed) / 1e9, m, len(os.sched_getaffinity(0))), flush=True)
        o1, o0, oc = (os.path.join(d, x) for x in ("bsub_out1", "bsub_out0", "bsub_outc"))
        series("subset -S -i, text path", [sub, "-S", "-i", refs, bed], 1, o1)
        if with_loop:
            series("subset -S -i, loop", [sub, "-S", "-i", refs, bed], 0, o0, reps=1)
            same = subprocess.run(["cmp", "-s", o1, o0]).returncode == 0
            print("outputs identical: %s (%d bytes)" % (same, os.path.getsize(o1)), flush=True)
            if not same:
                sys.exit("text path and loop disagree")
        series("subset -S -i -inv, text path", [sub, "-S", "-i", "-inv", refs, bed], 1, o1)
        series("count -S -i (same files)", [ovl, "count", "-S", "-i", refs, bed], 1, oc)
        if trace and shutil.which("rocprofv3"):
            kernel_stats([sub, "-S", "-i", refs, bed], dict(os.environ, GTX_TEXT_ON_DEVICE="1"), os.path.join(d, "bsub_prof_cli_%d" % nr), os.path.getsize(bed))
        for p in (bed, o1, o0, oc):
            if os.path.exists(p):
                os.remove(p)
    os.remove(refs)


GROUPS = (("tokenize", ("nl_count_kernel", "nl_scan_kernel", "nl_write_kernel", "text_parse_kernel", "text_void_kernel")), ("hits: narrow", ("query_narrow_kernel",)),
          ("verbatim", ("text_verbatim_kernel",)), ("select + gather", ("subset_mark_kernel", "subset_scan_kernel", "subset_gather_kernel")),
          ("hits: count walk", ("join_count_kernel",)), ("join scan + cut", ("scan_reduce_kernel", "scan_partials_kernel", "scan_apply_kernel", "join_cut")))


def kernel_stats(cmd, env, od, text_bytes=0):
    shutil.rmtree(od, ignore_errors=True)
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", od, "-o", "run", "--"] + cmd, stdout=subprocess.DEVNULL,
                           stderr=subprocess.PIPE, env=env, timeout=900)
    except subprocess.TimeoutExpired:
        sys.exit("the profiled run timed out")
    if r.returncode != 0:
        sys.exit("the profiled run failed (rc %d): %s" % (r.returncode, r.stderr.decode()[-2000:]))
    stats = glob.glob(os.path.join(od, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        print("no kernel stats written"); return
    rows = list(csv.DictReader(open(stats[0])))
    for gname, keys in GROUPS:
        sel = [x for x in rows if any(k in x["Name"] for k in keys)]
        if sel:
            ns = sum(float(x["TotalDurationNs"]) for x in sel); calls = sum(int(x["Calls"]) for x in sel)
            print("  kernels, %-16s total %9.3f ms in %5d launches%s" % (gname, ns / 1e6, calls, "  (%.1f GB/s of text)" % (text_bytes / ns) if text_bytes else ""), flush=True)
    other = [x for x in rows if not any(k in x["Name"] for _, keys in GROUPS for k in keys)]
    for x in sorted(other, key=lambda x: -float(x["TotalDurationNs"]))[:4]:
        print("  kernels, other: %-60s total %9.3f ms in %5s launches" % (x["Name"][:60], float(x["TotalDurationNs"]) / 1e6, x["Calls"]), flush=True)


if "--cli-only" not in sys.argv:
    passes()
    if trace and shutil.which("rocprofv3") and "--passes-only" not in sys.argv:
        print("kernel times of one more run of part 1 (all launches of its %d + 2 calls per entry and input):" % REPS, flush=True)
        kernel_stats([sys.executable, os.path.abspath(__file__), str(n), str(m), "--passes-only"], dict(os.environ), os.path.join(d, "bsub_prof_passes"))
if "--passes-only" not in sys.argv:
    cli()
