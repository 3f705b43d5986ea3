#!/usr/bin/env python3
"""The overlap join (gtx_join_device) on BASELINE config 3's shape: 100M reads resident in HBM x 1M refs, sorted-merge rules
(-S -i: ordinal order, no segment sort), reads sorted and shuffled.  Per order: the whole call (count + scan + emit, HIP events
around it), pairs/s, bytes moved against the algorithmic minimum (12 B per read read twice, 4 B count, 8 B offset, 4 B per pair)
and the fraction of the ~6.3 TB/s streaming ceiling; per-kernel times come from a `rocprofv3 --kernel-trace --stats` run of this
script.  Checked against the oracle: the per-region totals of the pairs of the first 2M reads equal the oracle's count."""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(R, "ibm-cbc-genomic-tools_amd")); sys.path.insert(0, R)
import numpy as np, torch, gtx
from gtx import synth
from bench import make_reads_on_device
from oracle import orc

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda", 0)
refs = synth.genome_intervals(1_000_000, 43, 50, 2000)
reads_sorted = make_reads_on_device(n, np.arange(24), 1000, dev)
n = reads_sorted.shape[0]
eng = gtx.Engine(0)
eng.set_refs(refs, 24, gtx.REFS_KEEP_ZERO_LENGTH)
eng.set_stream(torch.cuda.current_stream().cuda_stream)
d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)

for name, reads in (("sorted", reads_sorted), ("shuffled", reads_sorted[torch.randperm(n, device=dev)].contiguous())):
    total, _, _ = eng.join_device(reads.data_ptr(), n, d_off.data_ptr(), 0, 0, gtx.ZERO_LENGTH_OK)
    d_pairs = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    ms = []
    for it in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tot, done, info = eng.join_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, gtx.ZERO_LENGTH_OK)
        b.record(); b.synchronize()
        assert tot == total and done == n
        if it:
            ms.append(a.elapsed_time(b))
    t = float(np.median(ms))
    bytes_min = 12.0 * n * 2 + 4.0 * n + 8.0 * n + 4.0 * total
    print("join %-8s %d reads x %d refs: %d pairs, whole call %.3f ms (median of %d), %.3g pairs/s, %.0f GB/s algorithmic = %.1f%% of 6.3 TB/s"
          % (name, n, len(refs), total, t, reps, total / (t * 1e-3), bytes_min / (t * 1e-3) / 1e9, 100.0 * bytes_min / (t * 1e-3) / 6.3e12))
    if name == "sorted":
        ns = min(n, 2_000_000)
        off = d_off.cpu().numpy()
        got = np.bincount(d_pairs[:int(off[ns])].cpu().numpy(), minlength=len(refs)).astype(np.uint64)
        want = orc.count(refs, reads[:ns].cpu().numpy(), algo=orc.SORTED_MERGE)
        print("pairs of the first %d reads, per region, equal the oracle's count:" % ns, bool(np.array_equal(got, want)))
    del d_pairs
eng.close()
