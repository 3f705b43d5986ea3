#!/usr/bin/env python3
"""The annotate pass (gtx_pair_annotate_device) at bench_offset.py's shape: 100M sorted reads resident in HBM x 1M genes with random
strands plus their 1M upstream regions (--upstream-max 10000, untrimmed), one reference set of 2M regions under the bin index's
rules and order key, -i.  Timed apart with HIP events (one warm-up round, then medians): the join (gtx_join_device), the annotate
pass under center and under overlap, and gtx_pair_offsets_device (-op 5p) over the same pairs in the same run -- the pass walks
the pairs twice (count, emit), each walk reading what the offset pass reads and writing at most 12 B per kept pair against 16, so
the figure to report against is "at most twice the offset pass".  A prefix of the kept CSR is held against a numpy restatement
of PrintAnnotations' rule.  Then `genomic_annotate -i` end to end on 10M BED test regions, file in, text out to a pipe (third
argument; 0: skip), process start to exit.  Per-kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script."""
import os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(R, "ibm-cbc-genomic-tools_amd")); sys.path.insert(0, R)
import numpy as np, torch, gtx
from gtx import synth
from bench import make_reads_on_device

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_cli = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
UPSTREAM = 10_000
dev = torch.device("cuda", 0)
genes = synth.genome_intervals(1_000_000, 43, 50, 2000).astype(np.int64)
strand = np.random.default_rng(7).integers(0, 2, size=len(genes))
minus = strand == 1
# CreateGenomicRegionSetAnnotator without bounds or trimming: '+' [max(start - max, 1), max(start - 1, 1)], '-' [stop + 1, stop + max]
up = np.stack([genes[:, 0], np.where(minus, genes[:, 2] + 1, np.maximum(genes[:, 1] - UPSTREAM, 1)),
               np.where(minus, genes[:, 2] + UPSTREAM, np.maximum(genes[:, 1] - 1, 1))], axis=1)
refs = np.concatenate((genes, up)).astype(np.int32)
strands = np.concatenate((strand, strand))
N = len(genes)


def bin_rank(t):
    """the bin index's order per set: the rank of (level, bin, -ordinal), bits 17,20,23,26 and one bin above them"""
    s, e = np.maximum(t[:, 1], 1), t[:, 2]
    level = np.full(len(s), 5, dtype=np.int64); b = np.zeros(len(s), dtype=np.int64)
    for li, bits in reversed(list(enumerate((17, 20, 23, 26, 60)))):
        same = (s >> bits) == (e >> bits)
        level = np.where(same, li, level); b = np.where(same, s >> bits, b)
    order = np.lexsort((-np.arange(len(s)), b, level))
    key = np.empty(len(s), dtype=np.int64); key[order] = np.arange(len(s))
    return key


key = np.concatenate((bin_rank(genes), N + bin_rank(up)))
reads = make_reads_on_device(n, np.arange(24), 1000, dev)
n = reads.shape[0]
eng = gtx.Engine(0)
eng.set_refs(refs, 24)
eng.set_ref_order(key)
eng.set_ref_strands(strands)
eng.set_stream(torch.cuda.current_stream().cuda_stream)
d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
d_koff = torch.zeros(n + 1, dtype=torch.int64, device=dev)


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = f(); b.record(); b.synchronize()
    return a.elapsed_time(b), r


total, _, _ = eng.join_device(reads.data_ptr(), n, d_off.data_ptr(), 0, 0, gtx.JOIN_GAPS)
d_pairs = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
d_ref = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
d_val = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
d_out = torch.empty((max(total, 1), 2), dtype=torch.int64, device=dev)
tj, tc, ts, to = [], [], [], []
for it in range(reps + 1):
    t1, (tot, done, _) = timed(lambda: eng.join_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, gtx.JOIN_GAPS))
    assert tot == total and done == n
    t3, kept_s = timed(lambda: eng.pair_annotate_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, N, d_koff.data_ptr(),
                                                        d_ref.data_ptr(), d_val.data_ptr(), total, gtx.ANNOTATE_START))
    t4, inv = timed(lambda: eng.pair_offsets_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, d_out.data_ptr(), "5p"))
    t2, kept = timed(lambda: eng.pair_annotate_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, N, d_koff.data_ptr(),
                                                      d_ref.data_ptr(), d_val.data_ptr(), total, gtx.ANNOTATE_CENTER))
    assert kept_s == total and inv == -1
    if it:
        tj.append(t1); tc.append(t2); ts.append(t3); to.append(t4)
j, c, s, o = (float(np.median(x)) for x in (tj, tc, ts, to))
print("annotate %d reads x (%d genes + %d upstream regions): %d pairs, %d kept under center; join %.3f ms, annotate pass %.3f ms (center) / %.3f ms "
      "(overlap: every pair kept), offset pass over the same pairs %.3f ms (medians of %d after a warm-up round, HIP events around each call); "
      "ratio annotate / offset %.2f (center), %.2f (overlap)" % (n, N, len(up), total, kept, j, c, s, o, reps, c / o, s / o))
# a prefix against numpy: the first 1M reads' pairs
ns = min(n, 1_000_000)
off = d_off[:ns + 1].cpu().numpy(); koff = d_koff[:ns + 1].cpu().numpy()
p = d_pairs[:int(off[ns])].cpu().numpy().astype(np.int64)
q = np.repeat(np.arange(ns), np.diff(off))
rd = reads[:ns].cpu().numpy().astype(np.int64)
r64 = refs.astype(np.int64)
back = (strands[p] == 1) != (p >= N)                                            # -5p and +3p: the stop, offsets reversed
point = np.where(back, r64[p, 2], r64[p, 1])
total_off = np.where(back, 2 * point - rd[q, 1] - rd[q, 2], rd[q, 1] + rd[q, 2] - 2 * point)
keep = total_off >= 0
print("kept offsets, ordinals and values of the first %d reads (%d pairs, %d kept) equal the numpy restatement:" % (ns, len(p), int(keep.sum())),
      bool(np.array_equal(koff, np.concatenate(([0], np.cumsum(np.bincount(q[keep], minlength=ns))))) and
           np.array_equal(d_ref[:int(koff[ns])].cpu().numpy(), p[keep]) and np.array_equal(d_val[:int(koff[ns])].cpu().numpy(), total_off[keep])))
del d_pairs, d_out, d_ref, d_val
eng.close()

if n_cli > 0:
    tool = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_annotate")
    rd = reads[:n_cli].cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        def bed(path, t, st, prefix):
            with open(path, "w") as f:
                f.write("".join("chr%02d\t%d\t%d\t%s%d\t0\t%s\n" % (c, s - 1, e, prefix, i, "+-"[k]) for i, (c, s, e, k) in
                                enumerate(zip(t[:, 0].tolist(), t[:, 1].tolist(), t[:, 2].tolist(), st.tolist()))))
        bed(os.path.join(d, "genes.bed"), genes, strand, "g")
        bed(os.path.join(d, "reads.bed"), rd, np.zeros(len(rd), dtype=np.int64), "q")
        t0 = time.perf_counter()
        a = subprocess.Popen([tool, "-i", "genes.bed", "reads.bed"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        w = subprocess.Popen(["wc", "-l"], stdin=a.stdout, stdout=subprocess.PIPE)
        a.stdout.close()
        err = a.stderr.read(); a.wait()
        dt = time.perf_counter() - t0
        lines = int(w.communicate()[0])
        assert a.returncode == 0, err.decode()[-500:]
        print("genomic_annotate -i: %d BED test regions x %d genes (+ %d upstream regions) -> %d lines in %.2f s (process start to exit)"
              % (len(rd), len(genes), len(up), lines, dt))
