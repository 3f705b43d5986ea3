#!/usr/bin/env python3
"""Pair offsets (gtx_pair_offsets_device) on the pairs of the overlap join, BASELINE config 3's shape: 100M reads resident in
HBM x 1M refs with random strands, sorted-merge rules (-S -i), reads sorted and shuffled.  Per order: the join (gtx_join_device)
and the offset pass (-op 5p) timed apart with HIP events, the offset pass's bytes against the ~6.3 TB/s streaming ceiling --
per pair 4 B ordinal + 12 B gathered query triple + 16 B front / back interval + 1 B strand + 16 B out, and per query the two
8 B offsets its lane reads -- and a prefix of the output against a numpy restatement of GetOffsetFrom.  Then
`genomic_overlaps offset -i` (and -S -i) end to end on 10M BED reads, file in, text out to a pipe (third argument; 0: skip).  Per-kernel times come from a
`rocprofv3 --kernel-trace --stats` run of this script."""
import os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(R, "ibm-cbc-genomic-tools_amd")); sys.path.insert(0, R)
import numpy as np, torch, gtx
from gtx import synth
from bench import make_reads_on_device

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_cli = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
dev = torch.device("cuda", 0)
refs = synth.genome_intervals(1_000_000, 43, 50, 2000)
strand = np.random.default_rng(7).integers(0, 2, size=len(refs))
reads_sorted = make_reads_on_device(n, np.arange(24), 1000, dev)
n = reads_sorted.shape[0]
eng = gtx.Engine(0)
eng.set_refs(refs, 24, gtx.REFS_KEEP_ZERO_LENGTH)
eng.set_ref_strands(strand)
eng.set_stream(torch.cuda.current_stream().cuda_stream)
d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = f(); b.record(); b.synchronize()
    return a.elapsed_time(b), r


for name, reads in (("sorted", reads_sorted), ("shuffled", reads_sorted[torch.randperm(n, device=dev)].contiguous())):
    total, _, _ = eng.join_device(reads.data_ptr(), n, d_off.data_ptr(), 0, 0, gtx.ZERO_LENGTH_OK)
    d_pairs = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    d_out = torch.empty((max(total, 1), 2), dtype=torch.int64, device=dev)
    tj, to = [], []
    for it in range(reps + 1):
        t1, (tot, done, _) = timed(lambda: eng.join_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, gtx.ZERO_LENGTH_OK))
        assert tot == total and done == n
        t2, inv = timed(lambda: eng.pair_offsets_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, d_out.data_ptr(), "5p"))
        assert inv == -1
        if it:
            tj.append(t1); to.append(t2)
    j, o = float(np.median(tj)), float(np.median(to))
    b_pair, b_query = 49.0 * total, 16.0 * n
    print("offset %-8s %d reads x %d refs: %d pairs; join %.3f ms, offset pass %.3f ms (medians of %d, HIP events around each call), "
          "%.0f GB/s on %.2f GB per pair + %.2f GB offsets = %.1f%% of 6.3 TB/s"
          % (name, n, len(refs), total, j, o, reps, (b_pair + b_query) / (o * 1e-3) / 1e9, b_pair / 1e9, b_query / 1e9,
             100.0 * (b_pair + b_query) / (o * 1e-3) / 6.3e12))
    # a prefix against numpy: the first 2M reads' pairs, GetOffsetFrom with -op 5p on single-interval refs
    ns = min(n, 2_000_000)
    off = d_off[:ns + 1].cpu().numpy()
    p = d_pairs[:int(off[ns])].cpu().numpy().astype(np.int64)
    q = np.repeat(np.arange(ns), np.diff(off))
    rd = reads[:ns].cpu().numpy().astype(np.int64)
    minus = strand[p] == 1
    ref = np.where(minus, refs[p, 2], refs[p, 1]).astype(np.int64)
    want = np.where(minus[:, None], np.stack([ref - rd[q, 2], ref - rd[q, 1]], 1), np.stack([rd[q, 1] - ref, rd[q, 2] - ref], 1))
    print("offsets of the pairs of the first %d reads (%d pairs) equal the numpy restatement:" % (ns, len(p)),
          bool(np.array_equal(d_out[:len(p)].cpu().numpy(), want)))
    del d_pairs, d_out
eng.close()

# genomic_overlaps offset -i end to end: the first n_cli sorted reads as BED text (chromosome names whose strcmp order is the
# class order, so that -S sees sorted files)
if n_cli > 0:
    tool = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_overlaps")
    rd = reads_sorted[:n_cli].cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        def bed(path, t, st, prefix):
            with open(path, "w") as f:
                f.write("".join("chr%02d\t%d\t%d\t%s%d\t0\t%s\n" % (c, s - 1, e, prefix, i, "+-"[k]) for i, (c, s, e, k) in
                                enumerate(zip(t[:, 0].tolist(), t[:, 1].tolist(), t[:, 2].tolist(), st.tolist()))))
        bed(os.path.join(d, "refs.bed"), refs, strand, "r")
        bed(os.path.join(d, "reads.bed"), rd, np.zeros(len(rd), dtype=np.int64), "q")
        for args in (["-i"], ["-S", "-i"]):
            t0 = time.perf_counter()
            r = subprocess.run([tool, "offset"] + args + ["refs.bed", "reads.bed"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr.decode()[-500:]
            print("genomic_overlaps offset %s: %d BED reads x %d refs -> %d lines in %.2f s (process start to exit)"
                  % (" ".join(args), len(rd), len(refs), r.stdout.count(b"\n"), dt))
