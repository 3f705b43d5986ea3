#!/usr/bin/env python3
"""Signal bins (gtx_signal_bins_device): genomic_apps profile / heatmap's inner loop on 100M reads resident in HBM x 1M stranded
regions (synth.genome_intervals(..., stranded=True), strand-aware classes), each shifted 5000 nt upstream and downstream as the
reference shifts them, 100 bins over [-5000, 5000), reads sorted and shuffled.  Per order: the fused pass as profile (one row,
LDS-privatised) and as heatmap (n_refs x 100, global atomics), timed with HIP events (medians), against the unfused route on the
same regions -- the join (gtx_join_device) plus the offset pass (gtx_pair_offsets_device), which writes 4 B per pair, 8 B offsets
per read and 16 B offsets per pair and bins nothing yet.  Algorithmic bytes of the fused pass: 12 B per read triple + per pair
16 B front / back interval + 1 B strand (the index walk itself not counted), against the ~6.3 TB/s streaming ceiling.  The bins
of the first 2M reads are checked against a numpy restatement of the x / z / bin arithmetic on the join's pairs.  Then
`genomic_apps profile` end to end on 10M BED reads (third argument; 0: skip; a heatmap's .dat of 1M rows x 100 bins is
1.3 GB of text, so the CLI heatmap is left out)."""
import os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(R, "ibm-cbc-genomic-tools_amd")); sys.path.insert(0, R)
import numpy as np, torch, gtx
from gtx import synth
from bench import make_reads_on_device

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_cli = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
UP = DOWN = 5000
NB = 100
dev = torch.device("cuda", 0)
refs = synth.genome_intervals(1_000_000, 43, 50, 2000, stranded=True)
minus = refs[:, 0] >= 24
sh = refs.copy()
sh[:, 1] -= UP; sh[:, 2] += DOWN                          # single intervals: the 5' and 3' shifts together, either strand
half = make_reads_on_device(n // 2, np.arange(24), 1000, dev)   # classes 0-23 ('+'), then the same reads on 24-47 ('-')
other = half.clone(); other[:, 0] += 24
reads_sorted = torch.cat([half, other]).contiguous()
del half, other
n = reads_sorted.shape[0]
eng = gtx.Engine(0)
eng.set_refs(sh, 48)
eng.set_ref_strands(np.where(minus, "-", "+").tolist())
eng.set_signal_bins(-UP, DOWN, NB)
eng.set_stream(torch.cuda.current_stream().cuda_stream)
d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = f(); b.record(); b.synchronize()
    return a.elapsed_time(b), r


def restated(rd, off, p):
    q = np.repeat(np.arange(len(rd)), np.diff(off))
    m = minus[p]
    a = np.where(m, sh[p, 2].astype(np.int64) - rd[q, 2], rd[q, 1] - sh[p, 1].astype(np.int64))
    b = np.where(m, sh[p, 2].astype(np.int64) - rd[q, 1], rd[q, 2] - sh[p, 1].astype(np.int64))
    x = (a + b).astype(np.float64) / 2 / 1.0 + float(-UP)
    z = (x - float(-UP)) / (float(DOWN) - float(-UP))
    ok = (z >= 0) & (z < 1)
    k = (float(NB) * z[ok]).astype(np.int64)
    keep = k < NB
    return p[ok][keep], k[keep]


d_prof = torch.zeros(NB, dtype=torch.int64, device=dev)
d_heat = torch.zeros(len(sh) * NB, dtype=torch.int64, device=dev)
for name, reads in (("sorted", reads_sorted), ("shuffled", reads_sorted[torch.randperm(n, device=dev)].contiguous())):
    total, _, _ = eng.join_device(reads.data_ptr(), n, d_off.data_ptr(), 0, 0)
    d_pairs = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    d_out = torch.empty((max(total, 1), 2), dtype=torch.int64, device=dev)
    tp, th, tj, to = [], [], [], []
    for it in range(reps + 1):
        d_prof.zero_(); d_heat.zero_()
        t1, (inv, info) = timed(lambda: eng.signal_bins_device(reads.data_ptr(), n, d_prof.data_ptr(), None, 0))
        assert inv == -1 and info["n_pairs"] == total
        t2, (inv, _) = timed(lambda: eng.signal_bins_device(reads.data_ptr(), n, d_heat.data_ptr(), None, gtx.SIGNAL_PER_REF))
        t3, (tot, done, _) = timed(lambda: eng.join_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total))
        assert tot == total and done == n
        t4, inv = timed(lambda: eng.pair_offsets_device(reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, d_out.data_ptr(), "5p"))
        if it:
            tp.append(t1); th.append(t2); tj.append(t3); to.append(t4)
    p_, h_, j_, o_ = (float(np.median(v)) for v in (tp, th, tj, to))
    byt = 12.0 * n + 17.0 * total
    print("signal %-8s %d reads x %d refs: %d pairs, %d binned; profile %.3f ms (%.2f Gpairs/s, %.0f GB/s = %.1f%% of 6.3 TB/s), "
          "heatmap %.3f ms; unfused join %.3f ms + offsets %.3f ms = %.3f ms (%.1fx the profile pass) (medians of %d, HIP events around each call)"
          % (name, n, len(sh), total, info["n_binned"], p_, total / (p_ * 1e-3) / 1e9, byt / (p_ * 1e-3) / 1e9, 100.0 * byt / (p_ * 1e-3) / 6.3e12,
             h_, j_, o_, j_ + o_, (j_ + o_) / p_, reps))
    # the first 2M reads against numpy on the join's pairs
    ns = min(n, 2_000_000)
    d_prof.zero_(); d_heat.zero_()
    eng.signal_bins_device(reads.data_ptr(), ns, d_prof.data_ptr(), None, 0)
    eng.signal_bins_device(reads.data_ptr(), ns, d_heat.data_ptr(), None, gtx.SIGNAL_PER_REF)
    off = d_off[:ns + 1].cpu().numpy()
    p, k = restated(reads[:ns].cpu().numpy().astype(np.int64), off, d_pairs[:int(off[ns])].cpu().numpy().astype(np.int64))
    want_p = np.bincount(k, minlength=NB)
    want_h = np.bincount(p * NB + k, minlength=len(sh) * NB)
    print("bins of the first %d reads (%d pairs) equal the numpy restatement: profile %s, heatmap %s" % (
        ns, int(off[ns]), bool(np.array_equal(d_prof.cpu().numpy(), want_p)), bool(np.array_equal(d_heat.cpu().numpy(), want_h))))
    del d_pairs, d_out
eng.close()

# genomic_apps profile -i end to end on the first n_cli sorted reads as BED text
if n_cli > 0:
    tool = os.path.join(R, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_apps")
    rd = reads_sorted[:n_cli].cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        def bed(path, t, st, prefix):
            with open(path, "w") as f:
                f.write("".join("chr%02d\t%d\t%d\t%s%d\t0\t%s\n" % (c % 24, s - 1, e, prefix, i, "+-"[k]) for i, (c, s, e, k) in
                                enumerate(zip(t[:, 0].tolist(), t[:, 1].tolist(), t[:, 2].tolist(), st.tolist()))))
        bed(os.path.join(d, "tss.bed"), refs, minus.astype(np.int64), "r")
        bed(os.path.join(d, "reads.bed"), rd, (rd[:, 0] >= 24).astype(np.int64), "q")
        for op, extra in (("profile", ["-legend", "L"]),):
            t0 = time.perf_counter()
            r = subprocess.run([tool, op, "-o", "out", "-colors", "red"] + extra + ["reads.bed", "tss.bed"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr.decode()[-500:]
            print("genomic_apps %s: %d BED reads x %d refs -> %d bytes of .dat in %.2f s (process start to exit)"
                  % (op, len(rd), len(refs), os.path.getsize(os.path.join(d, "out.dat")), dt))
