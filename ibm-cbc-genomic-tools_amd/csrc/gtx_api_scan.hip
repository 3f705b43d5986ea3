// gtx_api_scan.hip -- the C ABI's scans: gtx_scan* over reads on the device, in host buffers or fed as a stream, the window vectors
// kept in HBM, the window selection, the window filter and the peak candidate selection over them, and their output lines as text.  Host code only (the kernels:
// gtx_kernels.hip, gtx_bucket.hip, gtx_scanown.hip, gtx_select.hip, gtx_filter.hip, gtx_peaks.hip, gtx_lines.hip); the context and the helpers shared
// with the other families are in gtx_ctx.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <cmath>
#include <chrono>
#include <algorithm>
#include <string>
#include <vector>
#include "gtx.h"
#include "gtx_kernels.h"
#include "gtx_select.h"
#include "gtx_filter.h"
#include "gtx_peaks.h"
#include "gtx_lines.h"
#include "gtx_internal.h"
#include "gtx_ctx.h"

extern "C" {

// ---------------------------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------------------------
int64_t gtx_scan_n_windows(int64_t len, int64_t step, int64_t size)
{
  if (step <= 0 || size <= 0 || len < 0) return 0;
  int64_t n = len / step, comb = size / step;
  return n < comb ? 0 : n - comb + 1;
}

// ownTile > 0: also lay out the blocks of the owner-computes pass (ownTile windows each); *own receives its table
static int scan_prepare(gtx_ctx *c, const int32_t *classLen, int nClasses, int step, int size, const int64_t *classOff, gtx::ScanArgs *out,
                        int ownTile = 0, gtx::ScanOwn *own = nullptr)
{
  if (nClasses < 1 || !classLen || !classOff) return fail(c, GTX_E_ARG, "gtx_scan: bad class table");
  if (step <= 0 || size <= 0 || size % step) return fail(c, GTX_E_ARG, "gtx_scan: window size must be a positive multiple of window step");
  std::vector<long long> key;
  key.push_back(nClasses); key.push_back(step); key.push_back(size); key.push_back(ownTile);
  for (int i = 0; i < nClasses; i++) { key.push_back(classLen[i]); key.push_back(classOff[i]); }
  const size_t tabLen = (size_t)6 * nClasses + 3;
  if (key != c->scan.key) {
    std::vector<long long> tab(tabLen);
    long long *microOff = tab.data(), *nMicro = microOff + nClasses, *winOff = nMicro + nClasses, *outOff = winOff + nClasses + 1,
              *tileOff = outOff + nClasses, *blkOff = tileOff + nClasses + 1;
    long long mo = 0, wo = 0, to = 0, bo = 0;
    const long long tile = gtx::scan_window_tile();
    for (int i = 0; i < nClasses; i++) {
      long long nm = classLen[i] < 0 ? 0 : classLen[i] / step;
      long long nw = gtx_scan_n_windows(classLen[i] < 0 ? 0 : classLen[i], step, size);
      microOff[i] = mo; nMicro[i] = nm; winOff[i] = wo; outOff[i] = classOff[i]; tileOff[i] = to; blkOff[i] = bo;
      mo += nm; wo += nw; to += (nw + tile - 1) / tile;
      if (ownTile > 0) bo += (nw + ownTile - 1) / ownTile;
    }
    winOff[nClasses] = wo; tileOff[nClasses] = to; blkOff[nClasses] = bo;
    c->scan.totalTiles = to; c->scan.ownBlocks = bo;
    HIPCHK(c, c->scan.tab.reserve(tabLen));
    HIPCHK(c, c->scan.micro.reserve((size_t)mo + 1, (size_t)mo + 3));
    HIPCHK(c, c->scan.bounds.reserve((size_t)(2 * bo + 2)));
    if (!c->scan.flag) HIPCHK(c, c->scan.flag.alloc(1));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->scan.tab.get(), tab.data(), tabLen * sizeof(long long), hipMemcpyHostToDevice));
    c->scan.key = key; c->scan.totalMicro = mo; c->scan.totalWindows = wo;
  }
  out->micro = c->scan.micro.get(); out->microOff = c->scan.tab.get(); out->nMicro = c->scan.tab.get() + nClasses;
  out->winOff = c->scan.tab.get() + 2 * nClasses; out->outOff = c->scan.tab.get() + 3 * nClasses + 1; out->tileOff = c->scan.tab.get() + 4 * nClasses + 1;
  out->nClasses = nClasses; out->winStep = step; out->comb = size / step;
  out->winStepInv = step > 1 ? (unsigned)((1ull << 32) / (unsigned)step) : 0;
  if (own) { own->blkOff = c->scan.tab.get() + 5 * nClasses + 2; own->tile = ownTile; own->totalBlocks = c->scan.ownBlocks; own->bounds = c->scan.bounds.get(); own->flag = c->scan.flag.get(); }
  return GTX_OK;
}

// Bucket tables over the POSITIONS of a scan geometry, for reads in no particular order (gtx_bucket.hip: bucket_scanhist_kernel):
// a bucket is a run of consecutive micro-windows of one class -- at most ~2000 buckets in all, at least 16 k micro-windows each --
// and is counted in parts of scan_part_bins() micro-windows.  Built when the geometry (or weighted / not) changes.
static int scan_bucket_tables(gtx_ctx *c, const int32_t *classLen, int nClasses, int step, bool weighted)
{
  std::vector<long long> key = c->scan.key; key.push_back(weighted ? 1 : 0);
  if (key == c->scan.bktKey) return GTX_OK;
  c->scan.bktKey.clear(); c->scan.nParts = 0;
  c->scan.bkt = {}; c->scan.parts.reset();
  if (!c->scan.info) HIPCHK(c, c->scan.info.alloc(1));
  long long total = 0;
  for (int i = 0; i < nClasses; i++) total += classLen[i] < 0 ? 0 : classLen[i] / step;
  BucketCuts k;
  k.clsStart.assign(nClasses + 1, 0);
  std::vector<gtx::ScanPart> parts;
  const int bins = gtx::scan_part_bins(weighted);
  const long long per = gtx::scan_bucket_per(total, bins, gtx::route_knobs());      // micro-windows per bucket
  for (int cl = 0; cl < nClasses; cl++) {
    k.clsStart[cl] = (int32_t)k.posHi.size();
    const long long nm = classLen[cl] < 0 ? 0 : classLen[cl] / step;
    for (long long f = 0; f < nm; f += per) {
      const long long g = std::min(f + per, nm);
      k.posHi.push_back(g == nm ? INT32_MAX : (int32_t)(g * step));                // positions <= g * step lie in micro-windows < g
      k.eLo.push_back((int32_t)f); k.eHi.push_back((int32_t)g); k.sLo.push_back(0); k.sHi.push_back(0); k.cls.push_back(cl);
      for (long long m = f; m < g; m += bins) parts.push_back({(int)k.posHi.size() - 1, (int)m, (int)std::min<long long>(bins, g - m), 0});
    }
  }
  k.clsStart[nClasses] = (int32_t)k.posHi.size();
  const int nB = (int)k.posHi.size();
  if (!gtx::scan_bucket_tables_ok(nB, nClasses, total)) { c->scan.bktKey = key; return GTX_OK; }   // (bktS.nB == 0: the general kernels serve)
  int rc = build_bucket_tables(c, c->scan.bkt, k, nClasses, true); if (rc) return rc;
  if (c->scan.bkt.nB > 0) {
    HIPCHK(c, upload(c->scan.parts, parts.data(), parts.size()));
    c->scan.nParts = (int)parts.size();
  }
  c->scan.bktKey = key;
  return GTX_OK;
}

// whether the partition path serves a batch of a scan: reads in no order under the unsorted scanner's rule (the bin index's), tables
// for the geometry, and partition_plan's word
static int scan_partition_plan(gtx_ctx *c, const int *dW, int64_t n, const gtx::ScanArgs &a, const int32_t *classLen, bool unsorted,
                               gtx::BucketPlan *p, gtx::BucketWork *w, bool *yes)
{
  *yes = false;
  if (!unsorted || a.sortedRule || !gtx::partition_worth(n, c->bucketMinReads)) return GTX_OK;
  int rc = scan_bucket_tables(c, classLen, a.nClasses, a.winStep, dW != nullptr); if (rc) return rc;
  return partition_plan(c, c->scan.bkt, n, a.nClasses, dW != nullptr, p, w, yes);
}

// one batch of reads by the partition path: into the micro-window histogram (zeroed by the caller), or -- d_windows not null -- the
// parts write the windows themselves (gtx::launch_scan_bucketed)
static int scan_hist_bucketed(gtx_ctx *c, const void *dR, const int *dW, int64_t n, const gtx::ScanArgs &a, const gtx::BucketPlan &p, const gtx::BucketWork &w, u64 *d_windows)
{
  gtx::CountArgs ca = {};                                      // what the partition pass reads of it; its counts of dropped reads go nowhere
  ca.nClasses = a.nClasses; ca.zeroLenOk = 0; ca.coverRule = 1; ca.keyCenter = a.center; ca.info = c->scan.info.get(); ca.indexBase = 0;
  HIPCHK(c, gtx::launch_scan_bucketed(dR, dW, n, ca, a, c->scan.bkt.view(), w, p, c->scan.parts.get(), c->scan.nParts, c->stream, d_windows));
  return GTX_OK;
}

} // extern "C"

// one batch of reads into the micro-window histogram (zeroed by the caller): the partition path or the general kernel
int scan_hist_any(gtx_ctx *c, const void *dR, const int *dW, int64_t n, const gtx::ScanArgs &a, const int32_t *classLen, bool unsorted)
{
  gtx::BucketPlan p; gtx::BucketWork w; bool part;
  int rc = scan_partition_plan(c, dW, n, a, classLen, unsorted, &p, &w, &part); if (rc) return rc;
  if (part) return scan_hist_bucketed(c, dR, dW, n, a, p, w, nullptr);
  HIPCHK(c, gtx::launch_scan_hist(dR, dW, n, a, c->stream));
  return GTX_OK;
}

extern "C" {

// the scan of reads resident in HBM, enqueued: owner-computes when the caller says the reads are sorted (checked on the device; the
// general kernels follow as conditional launches and run only if the check fails), the general kernels otherwise
static int scan_launch(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, const int32_t *classLen, int32_t nClasses, int32_t step,
                       int32_t size, char prep, uint32_t flags, const int64_t *classOff, void *d_out, bool profile)
{
  const gtx::RouteKnobs &knobs = gtx::route_knobs();
  int64_t totalMicro = 0;
  for (int i = 0; i < nClasses; i++) totalMicro += classLen[i] < 0 ? 0 : classLen[i] / step;
  const int tile = gtx::scan_own_wanted((flags & GTX_READS_SORTED) != 0, prep == '1', n, knobs) ? gtx::scan_own_tile(n, totalMicro, size / step) : 0;
  gtx::ScanArgs a; gtx::ScanOwn own;
  int rc = scan_prepare(c, classLen, nClasses, step, size, classOff, &a, tile, &own); if (rc) return rc;
  a.center = prep == 'c'; a.sortedRule = (flags & GTX_ZERO_LENGTH_OK) ? 1 : 0;
  if (c->scan.totalWindows > 0 && !d_out) return fail(c, GTX_E_ARG, "gtx_scan: null output");
  const bool micro64 = d_weights != nullptr;
  const size_t microBytes = (size_t)c->scan.totalMicro * (micro64 ? 8 : 4);
  const int *runIf = nullptr;
  if (tile > 0 && own.totalBlocks > 0) {
    HIPCHK(c, hipMemsetAsync(c->scan.flag.get(), 0, sizeof(int), c->stream));
    if (profile) HIPCHK(c, prof_mark(c, 1, c->stream));
    HIPCHK(c, gtx::launch_scan_own(d_reads, d_weights, n, a, own, (u64 *)d_out, c->stream));
    if (profile) HIPCHK(c, prof_mark(c, 2, c->stream));
    runIf = c->scan.flag.get();
    if (microBytes) HIPCHK(c, gtx::launch_scan_zero(c->scan.micro.get(), (long long)microBytes, runIf, c->stream));
    HIPCHK(c, gtx::launch_scan_hist(d_reads, d_weights, n, a, c->stream, runIf));
  } else {
    // reads in no order through the partition path: its parts write the windows themselves (no micro-window array, no window pass)
    gtx::BucketPlan p; gtx::BucketWork w; bool part;
    rc = scan_partition_plan(c, (const int *)d_weights, n, a, classLen, (flags & GTX_READS_UNSORTED) != 0, &p, &w, &part); if (rc) return rc;
    const bool fused = part && gtx::scan_fused_ok(a.comb, gtx::scan_fused_max_comb(), c->scan.totalWindows, knobs);
    if (!fused && microBytes) HIPCHK(c, hipMemsetAsync(c->scan.micro.get(), 0, microBytes, c->stream));
    if (profile) HIPCHK(c, prof_mark(c, 1, c->stream));
    if (part) { rc = scan_hist_bucketed(c, d_reads, (const int *)d_weights, n, a, p, w, fused ? (u64 *)d_out : nullptr); if (rc) return rc; }
    else HIPCHK(c, gtx::launch_scan_hist(d_reads, d_weights, n, a, c->stream));
    if (profile) HIPCHK(c, prof_mark(c, 2, c->stream));
    if (fused) return GTX_OK;
  }
  HIPCHK(c, gtx::launch_scan_windows(c->scan.micro.get(), micro64, a, c->scan.totalTiles, (u64 *)d_out, c->stream, runIf));
  return GTX_OK;
}

// a host-buffer call's reads brought into ONE device buffer (pageable memory through the page-locked slots), so that the
// owner-computes scan can be a single launch over all of them
static int stage_resident(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, void **dR, int **dW)
{
  if (c->stage.directPending) { HIPCHK(c, hipStreamSynchronize(c->stage.copyStream)); c->stage.directPending = false; }
  const size_t bytes = (size_t)n * 12, nW = weights ? (size_t)n : 0;
  if (bytes > c->scan.resReads.cap || nW > c->scan.resWeights.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
    HIPCHK(c, c->scan.resReads.reserve(bytes));
    HIPCHK(c, c->scan.resWeights.reserve(nW));
  }
  const bool direct = is_pinned(reads) && (!weights || is_pinned(weights));
  const int64_t batch = c->batchReads;
  const size_t slotBytes = (size_t)std::min<int64_t>(n, batch) * 16;
  if (!direct && (slotBytes > c->stage.pin[0].cap || slotBytes > c->stage.pin[1].cap)) {
    HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
    for (int k = 0; k < 2; k++) HIPCHK(c, c->stage.pin[k].reserve(slotBytes));
    c->stage.slotBusy[0] = c->stage.slotBusy[1] = false;
  }
  // the kernels of the previous call (the context's stream) may still be reading the resident buffer
  HIPCHK(c, hipEventRecord(c->scan.evRes[0], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->stage.copyStream, c->scan.evRes[0], 0));
  for (int64_t off = 0; off < n; off += batch) {
    const int64_t cnt = std::min(batch, n - off);
    const char *srcR = (const char *)(reads + 3 * off), *srcW = (const char *)(weights ? weights + off : nullptr);
    int slot = -1;
    if (!direct) {
      slot = (int)(c->stage.seq++ & 1);
      if (c->stage.slotBusy[slot]) HIPCHK(c, hipEventSynchronize(c->stage.evCopied[slot]));      // the DMA out of this page-locked slot is done
      parallel_copy(c->stage.pin[slot].get(), srcR, (size_t)cnt * 12, c->stage.copyThreads);
      if (weights) parallel_copy(c->stage.pin[slot].get() + (size_t)cnt * 12, srcW, (size_t)cnt * 4, c->stage.copyThreads);
      srcR = c->stage.pin[slot].get(); srcW = c->stage.pin[slot].get() + (size_t)cnt * 12;
    }
    HIPCHK(c, hipMemcpyAsync((char *)c->scan.resReads.get() + (size_t)off * 12, srcR, (size_t)cnt * 12, hipMemcpyHostToDevice, c->stage.copyStream));
    if (weights) HIPCHK(c, hipMemcpyAsync(c->scan.resWeights.get() + off, srcW, (size_t)cnt * 4, hipMemcpyHostToDevice, c->stage.copyStream));
    if (slot >= 0) { HIPCHK(c, hipEventRecord(c->stage.evCopied[slot], c->stage.copyStream)); c->stage.slotBusy[slot] = true; }
  }
  c->stage.directPending = direct;
  HIPCHK(c, hipEventRecord(c->scan.evRes[1], c->stage.copyStream));                              // everything has arrived before the scan starts
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->scan.evRes[1], 0));
  *dR = c->scan.resReads.get(); *dW = weights ? c->scan.resWeights.get() : nullptr;
  return GTX_OK;
}

int gtx_scan_device(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, const int32_t *classLen, int32_t nClasses,
                    int32_t step, int32_t size, char prep, uint32_t flags, void *d_out, const int64_t *classOff)
{
  if (!c) return GTX_E_ARG;
  if (n < 0 || (n > 0 && !d_reads)) return fail(c, GTX_E_ARG, "gtx_scan_device: bad argument");
  if (prep != '1' && prep != 'c') return fail(c, GTX_E_ARG, "gtx_scan_device: preprocess operator must be '1' or 'c'");
  if (!d_weights && n >= (1ll << 32)) return fail(c, GTX_E_ARG, "gtx_scan_device: unweighted scans count in 32 bits per micro-window: at most 2^32-1 reads per call");
  HIPCHK(c, hipSetDevice(c->device));
  prof_begin(c);
  int rc = scan_launch(c, d_reads, d_weights, n, classLen, nClasses, step, size, prep, flags, classOff, d_out, c->prof.profThis); if (rc) return rc;
  HIPCHK(c, prof_end(c, c->stream));
  return GTX_OK;
}

// the whole scan of host reads enqueued, result left in the context's own output vector in HBM
int gtxi_scan_enqueue(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, const int32_t *classLen, int32_t nClasses,
                      int32_t step, int32_t size, char prep, uint32_t flags, const int64_t *classOff, void **d_out, int64_t *extent_out)
{
  if (n < 0 || (n > 0 && !reads)) return fail(c, GTX_E_ARG, "gtx_scan: bad argument");
  if (prep != '1' && prep != 'c') return fail(c, GTX_E_ARG, "gtx_scan: preprocess operator must be '1' or 'c'");
  if (!weights && n >= (1ll << 32)) return fail(c, GTX_E_ARG, "gtx_scan: unweighted scans count in 32 bits per micro-window: at most 2^32-1 reads per call");
  if (nClasses < 1 || !classLen || !classOff) return fail(c, GTX_E_ARG, "gtx_scan: bad class table");
  if (step <= 0 || size <= 0 || size % step) return fail(c, GTX_E_ARG, "gtx_scan: window size must be a positive multiple of window step");
  HIPCHK(c, hipSetDevice(c->device));
  // output layout in the caller's buffer is given by class_offsets: find its extent
  int64_t extent = 0;
  for (int i = 0; i < nClasses; i++) extent = std::max<int64_t>(extent, classOff[i] + gtx_scan_n_windows(classLen[i] < 0 ? 0 : classLen[i], step, size));
  int rc = ensure_out(c, (size_t)extent); if (rc) return rc;
  if (extent > 0) HIPCHK(c, hipMemsetAsync(c->out.get(), 0, (size_t)extent * sizeof(u64), c->stream));
  if ((flags & GTX_READS_SORTED) && prep == '1' && n > 0) {
    // sorted reads: all of them resident, one owner-computes launch (gtx_scanown.hip)
    void *dR = nullptr; int *dW = nullptr;
    rc = stage_resident(c, reads, weights, n, &dR, &dW); if (rc) return rc;
    rc = scan_launch(c, dR, dW, n, classLen, nClasses, step, size, prep, flags, classOff, c->out.get(), false); if (rc) return rc;
  } else {
    gtx::ScanArgs a;
    rc = scan_prepare(c, classLen, nClasses, step, size, classOff, &a); if (rc) return rc;
    a.center = prep == 'c'; a.sortedRule = (flags & GTX_ZERO_LENGTH_OK) ? 1 : 0;
    const bool micro64 = weights != nullptr;
    if (c->scan.totalMicro > 0) HIPCHK(c, hipMemsetAsync(c->scan.micro.get(), 0, (size_t)c->scan.totalMicro * (micro64 ? 8 : 4), c->stream));
    rc = stage_batches(c, reads, weights, n, [&](const void *dR, const int *dW, int64_t cnt, int64_t off) -> int {
      const bool unsorted = (flags & GTX_READS_UNSORTED) || host_reads_look_unsorted(reads + 3 * off, cnt);
      return scan_hist_any(c, dR, dW, cnt, a, classLen, unsorted);
    });
    if (rc) return rc;
    HIPCHK(c, gtx::launch_scan_windows(c->scan.micro.get(), micro64, a, c->scan.totalTiles, c->out.get(), c->stream));
  }
  *d_out = c->out.get(); *extent_out = extent;
  return GTX_OK;
}

int gtx_scan(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, const int32_t *classLen, int32_t nClasses,
             int32_t step, int32_t size, char prep, uint32_t flags, uint64_t *out, const int64_t *classOff)
{
  if (!c) return GTX_E_ARG;
  void *d = nullptr; int64_t extent = 0;
  int rc = gtxi_scan_enqueue(c, reads, weights, n, classLen, nClasses, step, size, prep, flags, classOff, &d, &extent); if (rc) return rc;
  if (extent > 0 && !out) return fail(c, GTX_E_ARG, "gtx_scan: null output");
  if (extent > 0) HIPCHK(c, hipMemcpyAsync(out, d, (size_t)extent * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
  return GTX_OK;
}

// ---- the same scan fed as a stream (genomic_scans on an input of any size: host batches, or text tokenised on the device) ----
// The micro-window histogram accumulates over the batches (general kernels; batches in no order through the partition path), the
// sliding sums follow at the end.  The all-at-once calls above stay what a caller with every read in hand uses: they can take the
// owner-computes pass.
int gtx_scan_begin(gtx_ctx *c, const int32_t *classLen, int32_t nClasses, int32_t step, int32_t size, char prep, uint32_t flags, int weighted,
                   const int64_t *classOff)
{
  if (!c) return GTX_E_ARG;
  if (prep != '1' && prep != 'c') return fail(c, GTX_E_ARG, "gtx_scan_begin: preprocess operator must be '1' or 'c'");
  if (nClasses < 1 || !classLen || !classOff) return fail(c, GTX_E_ARG, "gtx_scan_begin: bad class table");
  if (step <= 0 || size <= 0 || size % step) return fail(c, GTX_E_ARG, "gtx_scan_begin: window size must be a positive multiple of window step");
  if (c->scan.cur.open || c->streamOpen || c->covOpen) return fail(c, GTX_E_STATE, "gtx_scan_begin: a call is open");
  HIPCHK(c, hipSetDevice(c->device));
  int64_t extent = 0;
  for (int i = 0; i < nClasses; i++) extent = std::max<int64_t>(extent, classOff[i] + gtx_scan_n_windows(classLen[i] < 0 ? 0 : classLen[i], step, size));
  int rc = ensure_out(c, (size_t)extent); if (rc) return rc;
  if (extent > 0) HIPCHK(c, hipMemsetAsync(c->out.get(), 0, (size_t)extent * sizeof(u64), c->stream));
  ScanOpen &s = c->scan.cur;
  rc = scan_prepare(c, classLen, nClasses, step, size, classOff, &s.a); if (rc) return rc;
  s.a.center = prep == 'c'; s.a.sortedRule = (flags & GTX_ZERO_LENGTH_OK) ? 1 : 0;
  s.weighted = weighted != 0; s.classLen.assign(classLen, classLen + nClasses); s.extent = extent; s.prep = prep; s.flags = flags;
  if (c->scan.totalMicro > 0) HIPCHK(c, hipMemsetAsync(c->scan.micro.get(), 0, (size_t)c->scan.totalMicro * (s.weighted ? 8 : 4), c->stream));
  if (!s.labelSum) HIPCHK(c, s.labelSum.alloc(1));
  HIPCHK(c, hipMemsetAsync(s.labelSum.get(), 0, sizeof(unsigned long long), c->stream));
  s.open = true;
  return GTX_OK;
}

int gtx_scan_add(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, uint32_t flags)
{
  if (!c) return GTX_E_ARG;
  if (!c->scan.cur.open) return fail(c, GTX_E_STATE, "gtx_scan_add: gtx_scan_begin has not been called");
  if (n < 0 || (n > 0 && !reads) || (c->scan.cur.weighted && n > 0 && !weights) || (!c->scan.cur.weighted && weights)) return fail(c, GTX_E_ARG, "gtx_scan_add: bad argument (weights as announced to gtx_scan_begin)");
  HIPCHK(c, hipSetDevice(c->device));
  ScanOpen &s = c->scan.cur;
  return stage_batches(c, reads, weights, n, [&](const void *dR, const int *dW, int64_t cnt, int64_t off) -> int {
    const bool unsorted = (flags & GTX_READS_UNSORTED) || host_reads_look_unsorted(reads + 3 * off, cnt);
    return scan_hist_any(c, dR, dW, cnt, s.a, s.classLen.data(), unsorted);
  });
}

int gtx_scan_end(gtx_ctx *c, uint64_t *out, int64_t *labelSum)
{
  if (!c) return GTX_E_ARG;
  if (!c->scan.cur.open) return fail(c, GTX_E_STATE, "gtx_scan_end: gtx_scan_begin has not been called");
  ScanOpen &s = c->scan.cur;
  s.open = false;
  if (s.extent > 0 && !out) return fail(c, GTX_E_ARG, "gtx_scan_end: null output");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtx::launch_scan_windows(c->scan.micro.get(), s.weighted, s.a, c->scan.totalTiles, c->out.get(), c->stream));
  if (s.extent > 0) HIPCHK(c, hipMemcpyAsync(out, c->out.get(), (size_t)s.extent * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  unsigned long long sum = 0;
  HIPCHK(c, hipMemcpyAsync(&sum, s.labelSum.get(), sizeof sum, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
  if (labelSum) *labelSum = (int64_t)sum;
  return GTX_OK;
}

// gtx_scan_end with the windows left on the device: the sliding sums are written into the slot's own vector (zero first: class_offsets
// may leave gaps), nothing but the label sum comes to the host
int gtx_scan_end_keep(gtx_ctx *c, int slot, int64_t *labelSum)
{
  if (!c) return GTX_E_ARG;
  if (!c->scan.cur.open) return fail(c, GTX_E_STATE, "gtx_scan_end_keep: gtx_scan_begin has not been called");
  ScanOpen &s = c->scan.cur;
  s.open = false;                                                    // (a refused slot ends the scan too, like gtx_scan_end's null output)
  if (slot < 0 || slot >= GTX_SCAN_KEEP_SLOTS) return fail(c, GTX_E_ARG, "gtx_scan_end_keep: slot out of range");
  HIPCHK(c, hipSetDevice(c->device));
  if ((size_t)s.extent > c->scan.kept[slot].cap || !c->scan.kept[slot]) {
    HIPCHK(c, hipStreamSynchronize(c->stream));                      // a selection may still be reading what the slot held
    HIPCHK(c, c->scan.kept[slot].alloc((size_t)std::max<int64_t>(s.extent, 1)));
  }
  c->scan.keptLen[slot] = s.extent;
  if (s.extent > 0) HIPCHK(c, hipMemsetAsync(c->scan.kept[slot].get(), 0, (size_t)s.extent * sizeof(u64), c->stream));
  HIPCHK(c, gtx::launch_scan_windows(c->scan.micro.get(), s.weighted, s.a, c->scan.totalTiles, c->scan.kept[slot].get(), c->stream));
  unsigned long long sum = 0;
  HIPCHK(c, hipMemcpyAsync(&sum, s.labelSum.get(), sizeof sum, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
  if (labelSum) *labelSum = (int64_t)sum;
  return GTX_OK;
}

int gtx_scan_kept(gtx_ctx *c, int slot, void **d_ptr, int64_t *n_windows)
{
  if (!c) return GTX_E_ARG;
  if (slot < 0 || slot >= GTX_SCAN_KEEP_SLOTS) return fail(c, GTX_E_ARG, "gtx_scan_kept: slot out of range");
  if (!c->scan.kept[slot]) return fail(c, GTX_E_STATE, "gtx_scan_kept: the slot is empty");
  if (d_ptr) *d_ptr = c->scan.kept[slot].get();
  if (n_windows) *n_windows = c->scan.keptLen[slot];
  return GTX_OK;
}

int gtx_scan_kept_read(gtx_ctx *c, int slot, uint64_t *out)
{
  if (!c) return GTX_E_ARG;
  if (slot < 0 || slot >= GTX_SCAN_KEEP_SLOTS) return fail(c, GTX_E_ARG, "gtx_scan_kept_read: slot out of range");
  if (!c->scan.kept[slot]) return fail(c, GTX_E_STATE, "gtx_scan_kept_read: the slot is empty");
  const int64_t n = c->scan.keptLen[slot];
  if (n > 0 && !out) return fail(c, GTX_E_ARG, "gtx_scan_kept_read: null output");
  HIPCHK(c, hipSetDevice(c->device));
  if (n > 0) HIPCHK(c, hipMemcpyAsync(out, c->scan.kept[slot].get(), (size_t)n * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTX_OK;
}

int gtx_scan_drop(gtx_ctx *c, int slot)
{
  if (!c) return GTX_E_ARG;
  if (slot < -1 || slot >= GTX_SCAN_KEEP_SLOTS) return fail(c, GTX_E_ARG, "gtx_scan_drop: slot out of range");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < GTX_SCAN_KEEP_SLOTS; k++) if (slot == -1 || slot == k) { c->scan.kept[k].reset(); c->scan.keptLen[k] = 0; }
  return GTX_OK;
}

} // extern "C" (templates below)

// ---- the tile compactions (gtx_compact.h): window selection, window filter, peak candidates ----
// A device entry behind its argument checks: the passes' scratch for n_windows (a pass may still be reading what it held: a sync in
// front of a growth), launch(tileCount, tileBase) enqueued, the number kept fetched.  It returns with the stream idle.
template <class Launch>
static int compact_device(gtx_ctx *c, int64_t n_windows, int64_t *n_kept, Launch launch)
{
  CompactState &s = c->cmp;
  const size_t nt = (size_t)gtx::compact_tiles(n_windows);
  if (!s.total) HIPCHK(c, s.total.alloc(1));
  if (nt > s.count.cap || nt + 1 > s.base.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, s.count.reserve(nt)); HIPCHK(c, s.base.reserve(nt + 1));
  }
  HIPCHK(c, launch(s.count.get(), s.base.get()));
  HIPCHK(c, hipMemcpyAsync(s.total.get(), s.base.get() + nt, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_kept = *s.total.get();
  return GTX_OK;
}

// A host entry behind its argument checks: device(d_ordinals, d_rows), the device entry, into the context's buffers for `capacity`
// rows of rowBytes; then the first min(kept, capacity) ordinals and rows out.
template <class Device>
static int compact_host(gtx_ctx *c, int64_t capacity, size_t rowBytes, int64_t *ordinals, void *rows, int64_t *n_kept, Device device)
{
  CompactState &s = c->cmp;
  HIPCHK(c, hipSetDevice(c->device));
  if ((size_t)capacity > s.ord.cap || (size_t)capacity * rowBytes > s.rows.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, s.ord.reserve((size_t)capacity)); HIPCHK(c, s.rows.reserve((size_t)capacity * rowBytes));
  }
  int rc = device(s.ord.get(), s.rows.get()); if (rc) return rc;
  const size_t got = (size_t)std::min<int64_t>(*n_kept, capacity);
  if (got) {
    HIPCHK(c, hipMemcpy(ordinals, s.ord.get(), got * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(rows, s.rows.get(), got * rowBytes, hipMemcpyDeviceToHost));
  }
  return GTX_OK;
}

extern "C" {

// ---- window selection (gtx_select.hip) ----
int gtx_window_select_limits(int32_t *tile, int32_t *lds_max_w)
{
  if (tile) *tile = gtx::kSelectTile;
  if (lds_max_w) *lds_max_w = gtx::kSelectLdsMaxW;
  return GTX_OK;
}

int gtx_window_select_device(gtx_ctx *c, const void *const *d_tested, const void *const *d_control, int32_t n_tested, int64_t n_windows, int32_t W,
                             const int32_t *const *kcrit, int64_t capacity, void *d_ordinals, void *d_rows, int64_t *n_kept)
{
  if (!c) return GTX_E_ARG;
  if (n_tested < 1 || n_tested > gtx::kSelectMaxTested || !d_tested || !kcrit || !n_kept) return fail(c, GTX_E_ARG, "gtx_window_select: 1 to 4 tested vectors, their tables and n_kept are required");
  if (n_windows < 0 || W < 1 || W == INT32_MAX || capacity < 0) return fail(c, GTX_E_ARG, "gtx_window_select: bad window count, window size or capacity");
  int n_ctl = 0;
  for (int f = 0; f < n_tested; f++) n_ctl += d_control && d_control[f] ? 1 : 0;
  if (n_ctl != 0 && n_ctl != n_tested) return fail(c, GTX_E_ARG, "gtx_window_select: a control for every tested vector, or for none");
  const bool ctl = n_ctl > 0;
  gtx::SelectArgs a = {};
  for (int f = 0; f < n_tested; f++) {
    if (!kcrit[f]) return fail(c, GTX_E_ARG, "gtx_window_select: null table");
    a.tested[f] = (const u64 *)d_tested[f]; a.control[f] = ctl ? (const u64 *)d_control[f] : nullptr;
    if (n_windows > 0 && (!a.tested[f] || ((uintptr_t)a.tested[f] & 15) || ((uintptr_t)a.control[f] & 15))) return fail(c, GTX_E_ARG, "gtx_window_select: vectors must be 16-byte aligned device memory");
  }
  if (capacity > 0 && (!d_ordinals || !d_rows)) return fail(c, GTX_E_ARG, "gtx_window_select: null output");
  *n_kept = 0;
  if (n_windows == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t stride = ctl ? (size_t)W + 1 : 1;
  if (stride * n_tested > c->sel.tab.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->sel.tab.reserve(stride * n_tested));
  }
  // (the tables are pageable host memory: these copies return when the source has been read)
  for (int f = 0; f < n_tested; f++) HIPCHK(c, hipMemcpyAsync(c->sel.tab.get() + f * stride, kcrit[f], stride * sizeof(int), hipMemcpyHostToDevice, c->stream));
  a.tab = c->sel.tab.get(); a.nTested = n_tested; a.W = W; a.n = n_windows;
  return compact_device(c, n_windows, n_kept, [&](unsigned *count, long long *base) {
    return gtx::launch_window_select(a, count, base, capacity, (long long *)d_ordinals, (int *)d_rows, c->stream);
  });
}

int gtx_window_select(gtx_ctx *c, const void *const *d_tested, const void *const *d_control, int32_t n_tested, int64_t n_windows, int32_t W,
                      const int32_t *const *kcrit, int64_t capacity, int64_t *ordinals, int32_t *rows, int64_t *n_kept)
{
  if (!c) return GTX_E_ARG;
  if (capacity < 0 || (capacity > 0 && (!ordinals || !rows))) return fail(c, GTX_E_ARG, "gtx_window_select: null output");
  if (n_tested < 1 || n_tested > gtx::kSelectMaxTested) return fail(c, GTX_E_ARG, "gtx_window_select: 1 to 4 tested vectors, their tables and n_kept are required");
  const size_t cols = (size_t)n_tested * ((d_control && d_control[0]) ? 2 : 1);
  return compact_host(c, capacity, cols * sizeof(int), ordinals, rows, n_kept, [&](void *d_ordinals, void *d_rows) {
    return gtx_window_select_device(c, d_tested, d_control, n_tested, n_windows, W, kcrit, capacity, d_ordinals, d_rows, n_kept);
  });
}

// ---- window filter (gtx_filter.hip) ----
static_assert(GTX_FILTER_TILE == gtx::kFilterTile, "include/gtx.h names the filter's tile");

int gtx_window_refs(gtx_ctx *c, const int32_t *refs, int64_t n_refs, const int32_t *classLen, const int64_t *classOff, int32_t nClasses, int32_t step,
                    int32_t size)
{
  if (!c) return GTX_E_ARG;
  FilterState &f = c->flt;
  f.set = false;
  if (n_refs < 0 || n_refs >= (int64_t)INT32_MAX - 64 || (n_refs > 0 && !refs)) return fail(c, GTX_E_ARG, "gtx_window_refs: bad argument (n_refs < 2^31 - 64)");
  if (nClasses < 1 || nClasses >= INT32_MAX - 1 || !classLen || !classOff) return fail(c, GTX_E_ARG, "gtx_window_refs: bad class table");
  if (step <= 0 || size <= 0 || size % step) return fail(c, GTX_E_ARG, "gtx_window_refs: window size must be a positive multiple of window step");
  // the classes that have windows, in the order of their offsets
  struct Blk { int64_t off, end; int cls; };
  std::vector<Blk> blk;
  for (int i = 0; i < nClasses; i++) {
    const int64_t nw = gtx_scan_n_windows(classLen[i] < 0 ? 0 : classLen[i], step, size);
    if (nw == 0) continue;
    if (classOff[i] < 0 || classOff[i] > INT64_MAX - nw) return fail(c, GTX_E_ARG, "gtx_window_refs: bad class offset");
    blk.push_back({classOff[i], classOff[i] + nw, i});
  }
  std::sort(blk.begin(), blk.end(), [](const Blk &a, const Blk &b) { return a.off < b.off; });
  for (size_t k = 1; k < blk.size(); k++) if (blk[k].off < blk[k - 1].end) return fail(c, GTX_E_ARG, "gtx_window_refs: two classes share window ordinals");
  std::vector<long long> off(blk.size() + 1, 0), end(blk.size() + 1, 0);
  std::vector<int> cls(blk.size() + 1, 0);
  for (size_t k = 0; k < blk.size(); k++) { off[k] = blk[k].off; end[k] = blk[k].end; cls[k] = blk[k].cls; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));                          // a pass may still be reading what the buffers held
  HIPCHK(c, upload(f.blkOff, off.data(), off.size())); HIPCHK(c, upload(f.blkEnd, end.data(), end.size())); HIPCHK(c, upload(f.blkCls, cls.data(), cls.size()));
  HIPCHK(c, f.first.reserve((size_t)nClasses + 2));
  HIPCHK(c, f.start.grow((size_t)n_refs)); HIPCHK(c, f.runmax.grow((size_t)n_refs));
  if (n_refs == 0) HIPCHK(c, hipMemsetAsync(f.first.get(), 0, ((size_t)nClasses + 2) * sizeof(int), c->stream));
  else {
    const size_t n3 = 3 * (size_t)n_refs;
    HIPCHK(c, f.tri.reserve(n3)); HIPCHK(c, f.keyed.reserve(n3)); HIPCHK(c, f.sorted.reserve(n3)); HIPCHK(c, f.order.reserve((size_t)n_refs));
    if (!f.bad) HIPCHK(c, f.bad.alloc(1));
    // (the triples are pageable host memory: the copy returns when the source has been read)
    HIPCHK(c, hipMemcpyAsync(f.tri.get(), refs, n3 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(f.bad.get(), 0, sizeof(unsigned), c->stream));
    HIPCHK(c, gtx::launch_filter_prepare(f.tri.get(), n_refs, nClasses, f.keyed.get(), f.bad.get(), c->stream));
    int rc = gtx_sort_device(c, f.keyed.get(), n_refs, nClasses + 1, f.order.get(), f.sorted.get()); if (rc) return rc;
    HIPCHK(c, gtx::launch_filter_index(f.sorted.get(), n_refs, nClasses, f.first.get(), f.start.get(), f.runmax.get(), c->stream));
    unsigned bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, f.bad.get(), sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) return fail(c, GTX_E_RANGE, "gtx_window_refs: a class id outside [0, n_classes)");
  }
  f.nClasses = nClasses; f.nBlk = (int)blk.size(); f.step = step; f.size = size; f.extent = blk.empty() ? 0 : blk.back().end;
  f.set = true;
  return GTX_OK;
}

int gtx_window_filter_device(gtx_ctx *c, const void *d_windows, int64_t n_windows, uint64_t min_value, int64_t capacity, void *d_ordinals, void *d_values,
                             int64_t *n_kept)
{
  if (!c) return GTX_E_ARG;
  FilterState &f = c->flt;
  if (!f.set) return fail(c, GTX_E_STATE, "gtx_window_filter: gtx_window_refs has not been called");
  if (n_windows < 0 || capacity < 0 || !n_kept) return fail(c, GTX_E_ARG, "gtx_window_filter: bad window count or capacity, or no n_kept");
  if (n_windows > 0 && (!d_windows || ((uintptr_t)d_windows & 15))) return fail(c, GTX_E_ARG, "gtx_window_filter: the vector must be 16-byte aligned device memory");
  if (capacity > 0 && (!d_ordinals || !d_values)) return fail(c, GTX_E_ARG, "gtx_window_filter: null output");
  if (f.extent > n_windows) return fail(c, GTX_E_ARG, "gtx_window_filter: a class of the prepared geometry reaches beyond n_windows");
  *n_kept = 0;
  if (n_windows == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  gtx::FilterRefs r = {f.start.get(), f.runmax.get(), f.first.get(), f.blkOff.get(), f.blkEnd.get(), f.blkCls.get(), f.nBlk, f.step, f.size};
  return compact_device(c, n_windows, n_kept, [&](unsigned *count, long long *base) {
    return gtx::launch_window_filter(r, (const u64 *)d_windows, n_windows, min_value, count, base, capacity, (long long *)d_ordinals, (u64 *)d_values, c->stream);
  });
}

int gtx_window_filter(gtx_ctx *c, const void *d_windows, int64_t n_windows, uint64_t min_value, int64_t capacity, int64_t *ordinals, uint64_t *values,
                      int64_t *n_kept)
{
  if (!c) return GTX_E_ARG;
  FilterState &f = c->flt;
  if (!f.set) return fail(c, GTX_E_STATE, "gtx_window_filter: gtx_window_refs has not been called");
  if (capacity < 0 || (capacity > 0 && (!ordinals || !values))) return fail(c, GTX_E_ARG, "gtx_window_filter: null output");
  return compact_host(c, capacity, sizeof(u64), ordinals, values, n_kept, [&](void *d_ordinals, void *d_values) {
    return gtx_window_filter_device(c, d_windows, n_windows, min_value, capacity, d_ordinals, d_values, n_kept);
  });
}

// ---- peak candidates (gtx_peaks.hip) ----
static_assert(GTX_PEAK_TILE == gtx::kPeakTile, "include/gtx.h names the peak selection's tile");

int gtx_peak_select_device(gtx_ctx *c, const void *d_signal, const void *d_control, const void *d_uniq, int64_t n_windows, int64_t win_size,
                           int64_t min_reads, int norm, double p_ratio, int64_t capacity, void *d_ordinals, void *d_rows, int64_t *n_kept)
{
  if (!c) return GTX_E_ARG;
  if (n_windows < 0 || capacity < 0 || !n_kept) return fail(c, GTX_E_ARG, "gtx_peak_select: bad window count or capacity, or no n_kept");
  if (win_size < 1) return fail(c, GTX_E_ARG, "gtx_peak_select: the window size must be positive");
  if (norm && !(std::isfinite(p_ratio) && p_ratio > 0.0)) return fail(c, GTX_E_ARG, "gtx_peak_select: -norm needs a finite positive ratio");
  if (!d_signal || !d_control || ((uintptr_t)d_signal & 15) || ((uintptr_t)d_control & 15) || ((uintptr_t)d_uniq & 15))
    return fail(c, GTX_E_ARG, "gtx_peak_select: signal and control (and the mappability track) must be 16-byte aligned device memory");
  if (capacity > 0 && (!d_ordinals || !d_rows)) return fail(c, GTX_E_ARG, "gtx_peak_select: null output");
  *n_kept = 0;
  if (n_windows == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  gtx::PeakArgs a = {(const u64 *)d_signal, (const u64 *)d_control, (const u64 *)d_uniq, n_windows, win_size, min_reads,
                     norm ? (p_ratio < 1.0 ? 1 : 2) : 0, p_ratio};
  return compact_device(c, n_windows, n_kept, [&](unsigned *count, long long *base) {
    return gtx::launch_peak_select(a, count, base, capacity, (long long *)d_ordinals, (long long *)d_rows, c->stream);
  });
}

int gtx_peak_select(gtx_ctx *c, const void *d_signal, const void *d_control, const void *d_uniq, int64_t n_windows, int64_t win_size,
                    int64_t min_reads, int norm, double p_ratio, int64_t capacity, int64_t *ordinals, int64_t *rows, int64_t *n_kept)
{
  if (!c) return GTX_E_ARG;
  if (capacity < 0 || (capacity > 0 && (!ordinals || !rows))) return fail(c, GTX_E_ARG, "gtx_peak_select: null output");
  return compact_host(c, capacity, 3 * sizeof(long long), ordinals, rows, n_kept, [&](void *d_ordinals, void *d_rows) {
    return gtx_peak_select_device(c, d_signal, d_control, d_uniq, n_windows, win_size, min_reads, norm, p_ratio, capacity, d_ordinals, d_rows, n_kept);
  });
}

}  // extern "C"

extern "C" {

// ---- output lines (gtx_lines.hip) ----
static_assert(GTX_LINES_TILE == gtx::kLinesTile && GTX_LINES_MAX_NAME == gtx::kLinesMaxName, "include/gtx.h names the line renderer's tile and name limit");

static int decimal_digits(unsigned long long u) { int d = 1; while (u >= 10) { u /= 10; d++; } return d; }

int gtx_lines_layout(gtx_ctx *c, const int64_t *block_offset, int32_t n_blocks, const char *names_blob, const int32_t *name_off, const char *strand,
                     int64_t win_step, int64_t win_size)
{
  if (!c) return GTX_E_ARG;
  LinesState &s = c->lines;
  s.set = false;
  if (n_blocks < 1 || !block_offset || !name_off || !strand || (!names_blob && name_off[n_blocks] > 0)) return fail(c, GTX_E_ARG, "gtx_lines_layout: blocks, names and strands are required");
  if (win_step < 1 || win_size < 1 || win_step > INT32_MAX || win_size > INT32_MAX) return fail(c, GTX_E_ARG, "gtx_lines_layout: window step and size must be positive and below 2^31");
  if (block_offset[0] != 0 || name_off[0] < 0) return fail(c, GTX_E_ARG, "gtx_lines_layout: offsets start at 0");
  int maxLine = 0;
  for (int b = 0; b < n_blocks; b++) {
    const int64_t nb = block_offset[b + 1] - block_offset[b];
    const int len = name_off[b + 1] - name_off[b];
    if (nb < 0 || block_offset[b + 1] > (1ll << 40)) return fail(c, GTX_E_ARG, "gtx_lines_layout: block offsets must ascend and stay at or below 2^40");
    if (len < 0) return fail(c, GTX_E_ARG, "gtx_lines_layout: name offsets must ascend");
    if (len > gtx::kLinesMaxName) return fail(c, GTX_E_ARG, "gtx_lines_layout: a name is longer than GTX_LINES_MAX_NAME");
    if (strand[b] != '+' && strand[b] != '-') return fail(c, GTX_E_ARG, "gtx_lines_layout: a strand is '+' or '-'");
    const unsigned long long k = (unsigned long long)std::max<int64_t>(nb - 1, 0);
    maxLine = std::max(maxLine, 20 + 1 + len + 3 + decimal_digits(win_step * k + 1) + 1 + decimal_digits(win_step * k + win_size) + 1);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));                          // a pass may still be reading what the buffers held
  HIPCHK(c, upload(s.blockOff, (const long long *)block_offset, (size_t)n_blocks + 1));
  HIPCHK(c, upload(s.nameOff, (const int *)name_off, (size_t)n_blocks + 1));
  HIPCHK(c, s.names.alloc((size_t)std::max(name_off[n_blocks], 1)));
  if (name_off[n_blocks] > 0) HIPCHK(c, hipMemcpy(s.names.get(), names_blob, (size_t)name_off[n_blocks], hipMemcpyHostToDevice));
  HIPCHK(c, upload(s.strand, strand, (size_t)n_blocks));
  s.nBlocks = n_blocks; s.maxLine = maxLine; s.total = block_offset[n_blocks]; s.step = win_step; s.size = win_size;
  s.set = true;
  return GTX_OK;
}

int64_t gtx_lines_max_bytes(gtx_ctx *c)
{
  if (!c) return GTX_E_ARG;
  if (!c->lines.set) return fail(c, GTX_E_STATE, "gtx_lines_max_bytes: gtx_lines_layout has not been called");
  return c->lines.maxLine;
}

int gtx_set_lines_chunk(gtx_ctx *c, int64_t bytes)
{
  if (!c) return GTX_E_ARG;
  if (bytes < 1) return fail(c, GTX_E_ARG, "gtx_set_lines_chunk: a positive number of bytes");
  c->lines.chunkBytes = bytes;
  return GTX_OK;
}

} // extern "C"

// One range of the renderer enqueued on the context's stream behind its argument checks: count, the two prefix scans, emit, and the
// range's totals (lines, bytes, the all-ones word) on their way into totals[3 * slot ..].  ordinals null: the vector rule.
static int lines_enqueue(gtx_ctx *c, const void *d_ordinals, const void *d_values, int64_t first, int64_t count, int64_t limit, int64_t min_value, void *d_text, int slot,
                         bool emit = true)
{
  LinesState &s = c->lines;
  const size_t nt = (size_t)gtx::lines_tiles(first, first + count);
  if (!s.endWord) HIPCHK(c, s.endWord.alloc(1));
  if (!s.totals) HIPCHK(c, s.totals.alloc(6));
  if (nt > s.tileLines.cap || nt + 1 > s.baseLines.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, s.tileLines.reserve(nt)); HIPCHK(c, s.tileBytes.reserve(nt)); HIPCHK(c, s.baseLines.reserve(nt + 1)); HIPCHK(c, s.baseBytes.reserve(nt + 1));
  }
  gtx::LinesArgs a = {};
  a.L = {s.blockOff.get(), s.nameOff.get(), s.names.get(), s.strand.get(), s.nBlocks, s.maxLine, s.step, s.size};
  a.values = (const u64 *)d_values; a.ordinals = (const long long *)d_ordinals;
  a.first = first; a.end = first + count; a.limit = std::min<int64_t>(limit, s.total); a.minValue = min_value;
  a.tileLines = s.tileLines.get(); a.tileBytes = s.tileBytes.get(); a.baseBytes = s.baseBytes.get(); a.endWord = s.endWord.get(); a.text = (char *)d_text;
  if (emit) HIPCHK(c, hipMemsetAsync(s.endWord.get(), 0xff, sizeof(u64), c->stream));
  HIPCHK(c, gtx::launch_lines_count(a, c->stream));
  HIPCHK(c, gtx::launch_tile_prefix(s.tileLines.get(), (long long)nt, s.baseLines.get(), c->stream));
  HIPCHK(c, gtx::launch_tile_prefix(s.tileBytes.get(), (long long)nt, s.baseBytes.get(), c->stream));
  if (emit) HIPCHK(c, gtx::launch_lines_emit(a, c->stream));
  u64 *tot = s.totals.get() + 3 * slot;
  HIPCHK(c, hipMemcpyAsync(tot, s.baseLines.get() + nt, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tot + 1, s.baseBytes.get() + nt, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (emit) HIPCHK(c, hipMemcpyAsync(tot + 2, s.endWord.get(), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  return GTX_OK;
}

// ... and waited for.  An all-ones value in the range: the emit pass has rendered what lies in front of it (it reads the word); the
// lines and bytes of that part are counted once more with the limit at that ordinal.
static int lines_finish(gtx_ctx *c, const void *d_ordinals, const void *d_values, int64_t first, int64_t count, int64_t min_value, int slot, int64_t *n_lines,
                        int64_t *n_bytes, int64_t *end_at)
{
  const u64 *tot = c->lines.totals.get() + 3 * slot;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *end_at = tot[2] == ~0ull ? -1 : (int64_t)tot[2];
  if (*end_at >= 0) {
    int rc = lines_enqueue(c, d_ordinals, d_values, first, count, *end_at, min_value, nullptr, slot, false); if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *n_lines = (int64_t)tot[0]; *n_bytes = (int64_t)tot[1];
  return GTX_OK;
}

static int lines_check(gtx_ctx *c, const char *who, const void *d_ordinals, const void *d_values, int64_t first, int64_t count, bool pairs)
{
  if (!c->lines.set) { c->err = std::string(who) + ": gtx_lines_layout has not been called"; return GTX_E_STATE; }
  if (first < 0 || count < 0 || first > INT64_MAX - count) { c->err = std::string(who) + ": bad range"; return GTX_E_ARG; }
  if (count > 0 && (!d_values || ((uintptr_t)d_values & 15) || (pairs && (!d_ordinals || ((uintptr_t)d_ordinals & 15))))) { c->err = std::string(who) + ": the vectors must be 16-byte aligned device memory"; return GTX_E_ARG; }
  if (!pairs && first + count > c->lines.total) { c->err = std::string(who) + ": the range reaches beyond the layout's windows"; return GTX_E_ARG; }
  return GTX_OK;
}

static int lines_device(gtx_ctx *c, const char *who, const void *d_ordinals, const void *d_values, int64_t first, int64_t count, int64_t limit, int64_t min_value,
                        void *d_text, int64_t capacity, int64_t *n_lines, int64_t *n_bytes, int64_t *end_at, bool pairs)
{
  if (!c) return GTX_E_ARG;
  int rc = lines_check(c, who, d_ordinals, d_values, first, count, pairs); if (rc) return rc;
  if (!n_lines || !n_bytes || !end_at || capacity < 0) { c->err = std::string(who) + ": n_lines, n_bytes and end_at are required, and a capacity"; return GTX_E_ARG; }
  if (count > capacity / c->lines.maxLine) { c->err = std::string(who) + ": count x gtx_lines_max_bytes exceeds the capacity"; return GTX_E_ARG; }
  if (count > 0 && (!d_text || ((uintptr_t)d_text & 15))) { c->err = std::string(who) + ": the text buffer must be 16-byte aligned device memory"; return GTX_E_ARG; }
  *n_lines = 0; *n_bytes = 0; *end_at = -1;
  if (count == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  rc = lines_enqueue(c, d_ordinals, d_values, first, count, limit, min_value, d_text, 0); if (rc) return rc;
  return lines_finish(c, d_ordinals, d_values, first, count, min_value, 0, n_lines, n_bytes, end_at);
}

// The streaming entries: ranges of whole tiles through two device and two page-locked buffers.  Range r + 1 is enqueued before the
// sink is given range r - 1, behind the copy of r - 1 out of the device buffer it writes (an event the stream waits for).
static int lines_stream(gtx_ctx *c, const char *who, const void *d_ordinals, const void *d_values, int64_t n, int64_t limit, int64_t min_value, gtx_lines_sink sink,
                        void *user, int64_t *n_lines, int64_t *n_bytes, int64_t *end_at, bool pairs)
{
  if (!c) return GTX_E_ARG;
  int rc = lines_check(c, who, d_ordinals, d_values, 0, n, pairs); if (rc) return rc;
  if (!sink) { c->err = std::string(who) + ": a sink is required"; return GTX_E_ARG; }
  LinesState &s = c->lines;
  int64_t lines = 0, bytes = 0, ended = -1;
  if (n_lines) *n_lines = 0;
  if (n_bytes) *n_bytes = 0;
  if (end_at) *end_at = -1;
  if (n == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t per = std::max<int64_t>(1, s.chunkBytes / ((int64_t)s.maxLine * gtx::kLinesTile)) * gtx::kLinesTile;   // entries per range: whole tiles
  const size_t room = (size_t)std::min(per, n) * (size_t)s.maxLine;
  if (room > s.text[0].cap || room > s.pin[0].cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
    for (int k = 0; k < 2; k++) { HIPCHK(c, s.text[k].reserve(room)); HIPCHK(c, s.pin[k].reserve(room)); }
  }
  for (int k = 0; k < 2; k++) if (!s.evCopied[k]) HIPCHK(c, hipEventCreateWithFlags(&s.evCopied[k], hipEventDisableTiming));
  const int64_t ranges = (n + per - 1) / per;
  int64_t got[2] = {0, 0};                                             // the bytes of the ranges in the two page-locked buffers
  // GTX_LINES_TIMING=1: where the host waited -- for a range's passes, for its copy, in the sink -- on stderr when the stream ends
  static const bool timing = getenv("GTX_LINES_TIMING") != nullptr;
  double waited[3] = {0, 0, 0};
  auto timed = [&](int what, auto &&fn) { const auto t0 = std::chrono::steady_clock::now(); auto r = fn(); waited[what] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); return r; };
  auto sink_range = [&](int64_t r) -> int {
    const int k = (int)(r & 1);
    HIPCHK(c, timed(1, [&] { return hipEventSynchronize(s.evCopied[k]); }));
    if (got[k] > 0 && timed(2, [&] { return sink(user, s.pin[k].get(), (size_t)got[k]); }) != 0) {
      (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->stage.copyStream);
      c->err = std::string(who) + ": the sink refused the text"; return GTX_E_SINK;
    }
    return GTX_OK;
  };
  rc = lines_enqueue(c, d_ordinals, d_values, 0, std::min(per, n), limit, min_value, s.text[0].get(), 0); if (rc) return rc;
  int64_t last = ranges - 1;
  for (int64_t r = 0; r < ranges; r++) {
    const int k = (int)(r & 1);
    const int64_t first = r * per, count = std::min(per, n - first);
    int64_t nl = 0, nb = 0;
    rc = timed(0, [&] { return lines_finish(c, d_ordinals, d_values, first, count, min_value, k, &nl, &nb, &ended); }); if (rc) return rc;
    lines += nl; bytes += nb; got[k] = nb;
    if (nb > 0) HIPCHK(c, hipMemcpyAsync(s.pin[k].get(), s.text[k].get(), (size_t)nb, hipMemcpyDeviceToHost, c->stage.copyStream));
    HIPCHK(c, hipEventRecord(s.evCopied[k], c->stage.copyStream));
    if (ended >= 0) last = r;
    if (r < last) {
      if (r >= 1) HIPCHK(c, hipStreamWaitEvent(c->stream, s.evCopied[k ^ 1], 0));   // the copy of r - 1 out of the buffer r + 1 is rendered into
      rc = lines_enqueue(c, d_ordinals, d_values, first + per, std::min(per, n - first - per), limit, min_value, s.text[k ^ 1].get(), k ^ 1); if (rc) return rc;
    }
    if (r >= 1) { rc = sink_range(r - 1); if (rc) return rc; }
    if (r == last) break;
  }
  rc = sink_range(last); if (rc) return rc;
  if (timing) fprintf(stderr, "[gtx lines] %lld ranges, %lld lines, %lld bytes: waited %.3f s for the passes, %.3f s for the copies, %.3f s in the sink\n",
                      (long long)(last + 1), (long long)lines, (long long)bytes, waited[0], waited[1], waited[2]);
  if (n_lines) *n_lines = lines;
  if (n_bytes) *n_bytes = bytes;
  if (end_at) *end_at = ended;
  return GTX_OK;
}

extern "C" {

int gtx_window_lines_device(gtx_ctx *c, const void *d_windows, int64_t first, int64_t count, int64_t limit, int64_t min_value, void *d_text, int64_t capacity,
                            int64_t *n_lines, int64_t *n_bytes, int64_t *end_at)
{
  return lines_device(c, "gtx_window_lines_device", nullptr, d_windows, first, count, limit, min_value, d_text, capacity, n_lines, n_bytes, end_at, false);
}

int gtx_pair_lines_device(gtx_ctx *c, const void *d_ordinals, const void *d_values, int64_t first, int64_t count, int64_t limit, void *d_text, int64_t capacity,
                          int64_t *n_lines, int64_t *n_bytes, int64_t *end_at)
{
  return lines_device(c, "gtx_pair_lines_device", d_ordinals, d_values, first, count, limit, 0, d_text, capacity, n_lines, n_bytes, end_at, true);
}

int gtx_window_lines(gtx_ctx *c, const void *d_windows, int64_t n_windows, int64_t limit, int64_t min_value, gtx_lines_sink sink, void *user, int64_t *n_lines,
                     int64_t *n_bytes, int64_t *end_at)
{
  return lines_stream(c, "gtx_window_lines", nullptr, d_windows, n_windows, limit, min_value, sink, user, n_lines, n_bytes, end_at, false);
}

int gtx_pair_lines(gtx_ctx *c, const void *d_ordinals, const void *d_values, int64_t n, int64_t limit, gtx_lines_sink sink, void *user, int64_t *n_lines,
                   int64_t *n_bytes, int64_t *end_at)
{
  return lines_stream(c, "gtx_pair_lines", d_ordinals, d_values, n, limit, 0, sink, user, n_lines, n_bytes, end_at, true);
}

// the filter into the compactions' own result buffers (room for max(2^16, n / 64) windows, grown once to what the filter reports),
// the pair rule over them: neither ordinals nor values come to the host
int gtx_window_filter_lines(gtx_ctx *c, const void *d_windows, int64_t n_windows, uint64_t min_value, int64_t limit, gtx_lines_sink sink, void *user,
                            int64_t *n_lines, int64_t *n_bytes, int64_t *end_at)
{
  if (!c) return GTX_E_ARG;
  if (!c->lines.set) return fail(c, GTX_E_STATE, "gtx_window_filter_lines: gtx_lines_layout has not been called");
  CompactState &s = c->cmp;
  HIPCHK(c, hipSetDevice(c->device));
  int64_t cap = std::max<int64_t>(1 << 16, n_windows / 64), kept = 0;
  for (;;) {
    if ((size_t)cap > s.ord.cap || (size_t)cap * sizeof(u64) > s.rows.cap) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, s.ord.reserve((size_t)cap)); HIPCHK(c, s.rows.reserve((size_t)cap * sizeof(u64)));
    }
    int rc = gtx_window_filter_device(c, d_windows, n_windows, min_value, cap, s.ord.get(), s.rows.get(), &kept); if (rc) return rc;
    if (kept <= cap) break;
    cap = kept;
  }
  return lines_stream(c, "gtx_window_filter_lines", s.ord.get(), s.rows.get(), kept, limit, 0, sink, user, n_lines, n_bytes, end_at, true);
}

}  // extern "C"
