#!/usr/bin/env python3
"""GFF / GTF reads end to end: `genomic_overlaps count -S -i refs.bed reads.gtf` with the text tokenised on the device
(GTX_TEXT_ON_DEVICE=1) and by the host packer (=0), same binary, process start to exit, median of 5, beside the same reads as BED3;
outputs compared with each other.  With --trace, one run of each input under `rocprofv3 --kernel-trace --stats`: the parse kernel's
time and the bytes/s it reads.
Usage: bench_gff.py [n_lines] [feature_len] [n_refs] [--trace] [--dir D]"""
import csv, glob, os, shutil, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BIN = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 10_000_000
fl = int(args[1]) if len(args) > 1 else 100
m = int(args[2]) if len(args) > 2 else 1_000_000
trace = "--trace" in sys.argv
d = sys.argv[sys.argv.index("--dir") + 1] if "--dir" in sys.argv else os.environ.get("TMPDIR", "/tmp")
pack = os.path.join(BIN, "gtx_packtool")
refs, gtf, bed = os.path.join(d, "bg_refs.bed"), os.path.join(d, "bg_reads.gtf"), os.path.join(d, "bg_reads.bed")
t = time.perf_counter()
subprocess.run([pack, "synthrefs", str(m), "43", refs], check=True)
subprocess.run([pack, "synthgff", str(n), "44", gtf, str(fl)], check=True)
subprocess.run([pack, "synth", str(n), "44", bed, str(fl)], check=True)
print("inputs written in %.1f s: GTF %.3f GB (%d features of %d bp, %.0f B/line), BED %.3f GB, refs %.1f MB" % (
    time.perf_counter() - t, os.path.getsize(gtf) / 1e9, n, fl, os.path.getsize(gtf) / n, os.path.getsize(bed) / 1e9, os.path.getsize(refs) / 1e6), flush=True)
print("cores available: %d" % len(os.sched_getaffinity(0)), flush=True)
exe = os.path.join(BIN, "genomic_overlaps")


def once(path, on_device):
    env = dict(os.environ, GTX_TEXT_ON_DEVICE=str(on_device), GTX_TEXT_TRACE="1")
    t0 = time.perf_counter()
    try:
        r = subprocess.run([exe, "count", "-S", "-i", refs, path], capture_output=True, env=env, timeout=120)
    except subprocess.TimeoutExpired:
        sys.exit("timed out: %s" % path)                                  # (a GPU step that hangs or fails ends the run: nothing more is started)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("failed (rc %d): %s" % (r.returncode, r.stderr.decode()[-2000:]))
    tr = [l for l in r.stderr.decode().splitlines() if l.startswith("[gtx text]")]
    return dt, r.stdout, tr[0] if tr else "(host packer)"


outs = {}
for name, path, dev in (("GTF device", gtf, 1), ("GTF host  ", gtf, 0), ("BED device", bed, 1), ("BED host  ", bed, 0)):
    once(path, dev)                                                          # (page cache warm, first-run costs out)
    times = []
    for _ in range(5):
        dt, out, tr = once(path, dev)
        times.append(dt)
    outs[name] = out
    print("%s  count -S -i: %.3f s (median of 5; runs %s)  %s" % (name, sorted(times)[2], " ".join("%.3f" % x for x in times), tr), flush=True)
assert len(set(outs.values())) == 1, "outputs differ"
print("outputs identical (%d lines)" % outs["GTF device"].count(b"\n"), flush=True)

if trace and shutil.which("rocprofv3"):
    for name, path in (("GTF", gtf), ("BED", bed)):
        od = os.path.join(d, "bg_prof_" + name)
        shutil.rmtree(od, ignore_errors=True)
        env = dict(os.environ, GTX_TEXT_ON_DEVICE="1")
        try:
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", od, "-o", "run", "--", exe, "count", "-S", "-i", refs, path],
                               capture_output=True, env=env, timeout=180)
        except subprocess.TimeoutExpired:
            sys.exit("%s: the profiled run timed out" % name)
        if r.returncode != 0:
            sys.exit("%s: the profiled run failed (rc %d): %s" % (name, r.returncode, r.stderr.decode()[-2000:]))
        stats = glob.glob(os.path.join(od, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            print("%s: no kernel stats written" % name); continue
        size = os.path.getsize(path)
        for row in csv.DictReader(open(stats[0])):
            k = row["Name"]
            if any(x in k for x in ("text_parse_kernel", "nl_count_kernel", "nl_write_kernel")):
                ns = float(row["TotalDurationNs"])
                print("%s  %-70s calls %5s  total %9.3f ms  %7.2f GB/s of text" % (name, k[:70], row["Calls"], ns / 1e6, size / ns), flush=True)
for p in (gtf, bed, refs):
    os.remove(p)
