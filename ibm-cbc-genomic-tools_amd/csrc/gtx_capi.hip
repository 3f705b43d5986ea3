// gtx_capi.hip -- implementation of the C ABI declared in include/gtx.h: the context, the reference side, count and coverage.
//
// Host side of the engine: builds the device-resident rank structure from the reference
// regions (replacing the bin-index construction of UnsortedGenomicRegionSetOverlaps,
// gtools/genomic_intervals.cpp:5593-5675), enqueues the streaming count / coverage kernels of
// gtx_kernels.hip, and moves buffers.  There is deliberately no CPU implementation of the
// counting path in this library: without a HIP device every entry point fails.
//
// The context itself (struct gtx_ctx) and the helpers other families share are in gtx_ctx.h; the other families of entry points:
// gtx_api_join.hip (join, per-query hits, pair offsets, annotate, signal bins), gtx_api_scan.hip (scans, kept windows, window
// selection), gtx_api_text.hip (the text feed), gtx_api_link.hip (link and the neighbour passes).  Here: gtx_create .. gtx_n_refs,
// the reference set, count, the host-buffer staging, the pair corrections, coverage, the group's gtxi_* hooks, gtx_profile_*.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>
#include "gtx.h"
#include "gtx_kernels.h"
#include "gtx_pairs.h"
#include "gtx_internal.h"
#include "gtx_ctx.h"

static thread_local std::string g_create_error;

// histograms, tile sums, prefix arrays, chain flags and tile totals over histLen slots; histograms, tile sums, flags and totals zero
// (the invariant between calls: the finalize kernels leave them so -- of the totals, the ones the next call writes)
int make_hist_set(gtx_ctx *c, HistSet &h, int64_t histLen)
{
  const size_t parts = (size_t)gtx::scan_tiles(histLen) + 2;
  HIPCHK(c, h.histA.alloc(histLen)); HIPCHK(c, h.histB.alloc(histLen)); HIPCHK(c, h.partA.alloc(parts)); HIPCHK(c, h.partB.alloc(parts));
  HIPCHK(c, h.prefA.alloc(histLen)); HIPCHK(c, h.prefB.alloc(histLen)); HIPCHK(c, h.flags.alloc(8 * parts));
  HIPCHK(c, h.totals.alloc(4 * parts));
  for (DevBuf<u64> *b : {&h.histA, &h.histB, &h.partA, &h.partB, &h.totals}) HIPCHK(c, hipMemset(b->get(), 0, sizeof(u64) * b->cap));
  HIPCHK(c, hipMemset(h.flags.get(), 0, sizeof(unsigned) * h.flags.cap));
  h.epoch = 0; h.draws = 0; h.totalsTurn = 0;
  return GTX_OK;
}

// direct placement (gtx::PlaceTable) over two boundary arrays with the class segments `seg` (the same array twice for the
// coverage thresholds): cells of 2^sh positions, sh the smallest shift that keeps the table at about one cell per eight
// boundaries; a cell's entries = how many boundaries of the class lie below the cell's first position in either array (cell 0: none)
int make_place_table(gtx_ctx *c, const std::vector<int32_t> &seg, const std::vector<int32_t> &arrA, const std::vector<int32_t> &arrB,
                     int nClasses, int64_t nv, PlaceTable &out)
{
  const int64_t budget = std::max<int64_t>(1024, nv / 8) + 2 * (int64_t)nClasses;
  auto cellsOf = [&](int cl, int sh) -> int64_t {
    if (seg[cl] == seg[cl + 1]) return 0;
    const int64_t top = std::max<int64_t>(0, std::max(arrA[seg[cl + 1] - 1], arrB[seg[cl + 1] - 1]));
    return (top >> sh) + 2;
  };
  int sh = 0;
  for (;; sh++) { int64_t t = 0; for (int cl = 0; cl < nClasses; cl++) t += cellsOf(cl, sh); if (t <= budget || sh >= 31) break; }
  std::vector<int4> pc(std::max(nClasses, 1));
  std::vector<int32_t> rank;
  for (int cl = 0; cl < nClasses; cl++) {
    const int64_t nc = cellsOf(cl, sh);
    pc[cl] = make_int4(seg[cl], seg[cl + 1], (int)(rank.size() / 2), (int)nc);
    int32_t ia = seg[cl], ib = seg[cl];
    for (int64_t k = 0; k < nc; k++) {
      const int64_t first = k << sh;                           // cell 0 stands for everything below 2^sh, negative keys included
      if (k > 0) { while (ia < seg[cl + 1] && arrA[ia] < first) ia++; while (ib < seg[cl + 1] && arrB[ib] < first) ib++; }
      rank.push_back(ia); rank.push_back(ib);
    }
  }
  rank.push_back(0); rank.push_back(0);
  out.cls.reset(); out.rank.reset();
  HIPCHK(c, out.cls.alloc(pc.size()));
  HIPCHK(c, out.rank.alloc(rank.size()));
  HIPCHK(c, hipMemcpy(out.cls.get(), pc.data(), sizeof(int4) * pc.size(), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(out.rank.get(), rank.data(), sizeof(int32_t) * rank.size(), hipMemcpyHostToDevice));
  out.shift = sh;
  return GTX_OK;
}

// t = the tables of cuts k: cells over the span of each class's cuts, the shift that keeps all classes within 4096 cells, a cell's
// first bucket relative to its class's; uploaded if they fit the LDS of the scatter kernel (32 B per bucket, 16 per class), t.nB = 0
// otherwise.  sync: wait for the context's stream before the tables are made.
int build_bucket_tables(gtx_ctx *c, BucketTables &t, BucketCuts &k, int nClasses, bool sync)
{
  t.nB = 0;
  const int nB = (int)k.posHi.size();
  if (nB == 0) return GTX_OK;
  const std::vector<int32_t> &posHi = k.posHi, &clsStart = k.clsStart;
  const int kCells = 4096;
  int sh = 0;
  auto cellsAt = [&](int shift) {
    int64_t total = 0;
    for (int cl = 0; cl < nClasses; cl++) {
      const int b0 = clsStart[cl], b1 = clsStart[cl + 1];
      total += b1 - b0 <= 1 ? b1 - b0 : ((((int64_t)posHi[b1 - 2] - posHi[b0]) >> shift) + 1);
    }
    return total;
  };
  while (sh < 40 && cellsAt(sh) > kCells) sh++;
  std::vector<int32_t> clsCell(4 * (size_t)nClasses);
  std::vector<uint16_t> cellTab;
  for (int cl = 0; cl < nClasses; cl++) {
    const int b0 = clsStart[cl], b1 = clsStart[cl + 1];
    const int32_t lo = b1 - b0 <= 1 ? 0 : posHi[b0];
    const int64_t nc = b1 == b0 ? 0 : b1 - b0 == 1 ? 1 : ((((int64_t)posHi[b1 - 2] - lo) >> sh) + 1);   // 0 cells: a class without buckets
    clsCell[4 * cl] = (int32_t)cellTab.size(); clsCell[4 * cl + 1] = lo; clsCell[4 * cl + 2] = (int32_t)nc; clsCell[4 * cl + 3] = b0;
    int b = b0;
    for (int64_t j = 0; j < nc; j++) {
      const int64_t first = (int64_t)lo + (j << sh);
      while (b < b1 - 1 && (int64_t)posHi[b] < first) b++;
      cellTab.push_back((uint16_t)(b - b0));
    }
  }
  t.nCells = (int)cellTab.size(); t.cellShift = sh;
  if (!gtx::bucket_tables_fit(nClasses, nB, t.nCells)) return GTX_OK;
  cellTab.push_back(0);
  std::vector<int32_t> all;
  for (auto *v : {&k.posHi, &k.eLo, &k.eHi, &k.sLo, &k.sHi, &k.cls, &k.clsStart}) all.insert(all.end(), v->begin(), v->end());
  if (sync) HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, upload(t.bkt, all.data(), all.size()));
  HIPCHK(c, t.clsCell.alloc((size_t)nClasses + 1));                // (16 bytes beyond the last class)
  HIPCHK(c, hipMemcpy(t.clsCell.get(), clsCell.data(), sizeof(int32_t) * clsCell.size(), hipMemcpyHostToDevice));
  HIPCHK(c, upload(t.cellTab, cellTab.data(), cellTab.size()));
  t.nB = nB;
  return GTX_OK;
}

extern "C" {

int gtx_version(void) { return 100; }

gtx_ctx *gtx_create(int device_id)
{
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_error = std::string("gtx_create: no usable HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                     "); this library has no CPU path";
    return nullptr;
  }
  if (device_id < 0 || device_id >= n) { g_create_error = "gtx_create: device id out of range"; return nullptr; }
  if ((e = hipSetDevice(device_id)) != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return nullptr; }
  gtx_ctx *c = new gtx_ctx();
  c->device = device_id;
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->waveSlots = 32ll * cus; }
  if (c->d_info.alloc(2) != hipSuccess || c->h_info.alloc(2) != hipSuccess) {
    g_create_error = "gtx_create: allocation failed"; delete c; return nullptr;
  }
  gtx::DevInfo *hi = c->h_info.get();
  hi[1].first_unsorted = INT64_MAX; hi[1].n_no_class = 0; hi[1].n_degenerate = 0; hi[1].first_degenerate = INT64_MAX; hi[1].n_unplaced = 0; hi[1].fault = 0;
  hi[0] = hi[1];
  if (hipMemcpy(c->d_info.get(), &hi[1], sizeof(gtx::DevInfo), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_info.get() + 1, &hi[1], sizeof(gtx::DevInfo), hipMemcpyHostToDevice) != hipSuccess) {
    g_create_error = "gtx_create: hipMemcpy failed"; delete c; return nullptr;
  }
  for (auto &slot : c->prof.ring) for (auto &ev : slot) if (hipEventCreate(&ev) != hipSuccess) { g_create_error = "gtx_create: hipEventCreate failed"; delete c; return nullptr; }
  if (hipStreamCreateWithFlags(&c->stage.copyStream, hipStreamNonBlocking) != hipSuccess) { g_create_error = "gtx_create: hipStreamCreate failed"; delete c; return nullptr; }
  for (int k = 0; k < 2; k++)
    if (hipEventCreateWithFlags(&c->stage.evCopied[k], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->stage.evConsumed[k], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->scan.evRes[k], hipEventDisableTiming) != hipSuccess) {
      g_create_error = "gtx_create: hipEventCreate failed"; delete c; return nullptr;
    }
  { unsigned hc = std::thread::hardware_concurrency(); c->stage.copyThreads = (int)std::max(1u, std::min(hc ? hc : 4u, 8u));
    if (const char *ct = getenv("GTX_COPY_THREADS")) if (atoi(ct) > 0) c->stage.copyThreads = atoi(ct); }
  const char *cpw = getenv("GTX_CHUNKS_PER_WAVE");
  if (cpw && atoi(cpw) > 0) c->chunksPerWave = atoi(cpw);
  const char *br = getenv("GTX_BATCH_READS");
  if (br && atoll(br) > 0) c->batchReads = atoll(br);
  if (const char *bm = getenv("GTX_BUCKET_MIN_READS")) c->bucketMinReads = atoll(bm);   // unsorted reads: batches below this use the search kernel
  if (const char *lt = getenv("GTX_LOCAL_SCAN_MAX_TILES")) c->localMaxTiles = std::min(std::max(atoi(lt), 0), gtx::kLocalScanMaxTiles);
  return c;
}

void gtx_destroy(gtx_ctx *c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stage.copyStream) (void)hipStreamSynchronize(c->stage.copyStream);
  for (int k = 0; k < 2; k++)
    for (hipEvent_t e : {c->stage.evCopied[k], c->stage.evConsumed[k], c->scan.evRes[k]}) if (e) (void)hipEventDestroy(e);
  if (c->stage.copyStream) (void)hipStreamDestroy(c->stage.copyStream);
  for (auto &t : c->text.slot) for (hipEvent_t e : {t.evParsed, t.evConsumed, t.evCopied}) if (e) (void)hipEventDestroy(e);
  for (auto &slot : c->prof.ring) for (auto &ev : slot) if (ev) (void)hipEventDestroy(ev);
  delete c;
}

const char *gtx_last_error(const gtx_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int gtx_set_stream(gtx_ctx *c, void *s) { if (!c) return GTX_E_ARG; c->stream = (hipStream_t)s; return GTX_OK; }

int gtx_sync(gtx_ctx *c)
{
  if (!c) return GTX_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->link.mail.deliver(); c->nbr.adj.deliver(); c->nbr.gap.deliver();     // the info blocks of the last device calls have arrived
  return GTX_OK;
}

void *gtx_host_alloc(gtx_ctx *c, size_t bytes)
{
  if (!c) return nullptr;
  void *p = nullptr;
  // (portable: any device of a group may read it)
  if (hipSetDevice(c->device) != hipSuccess || hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { c->err = "gtx_host_alloc: hipHostMalloc failed"; (void)hipGetLastError(); return nullptr; }
  return p;
}

void gtx_host_free(gtx_ctx *c, void *p) { (void)c; if (p) (void)hipHostFree(p); }

int64_t gtx_n_refs(const gtx_ctx *c) { return c ? c->nRefs : -1; }

// ---------------------------------------------------------------------------------------------
// reference side
// ---------------------------------------------------------------------------------------------
int gtx_set_refs(gtx_ctx *c, const int32_t *tri, int64_t m, int32_t nClasses) { return gtx_set_refs_ex(c, tri, m, nClasses, 0); }

int gtx_set_refs_ex(gtx_ctx *c, const int32_t *tri, int64_t m, int32_t nClasses, uint32_t flags)
{
  if (!c || m < 0 || (m > 0 && !tri)) return c ? fail(c, GTX_E_ARG, "gtx_set_refs: bad argument") : GTX_E_ARG;
  if (m >= (int64_t)INT32_MAX - 4096) return fail(c, GTX_E_ARG, "gtx_set_refs: too many reference regions");
  HIPCHK(c, hipSetDevice(c->device));
  int maxc = -1;
  for (int64_t k = 0; k < m; k++) {
    int32_t cl = tri[3 * k], s = tri[3 * k + 1], e = tri[3 * k + 2];
    if (cl < -1) return fail(c, GTX_E_RANGE, "gtx_set_refs: negative class id");      // -1: a placeholder that never matches
    if (s >= INT32_MAX - 1 || e >= INT32_MAX - 1) return fail(c, GTX_E_RANGE, "gtx_set_refs: coordinate >= 2^31-2");
    if (cl > maxc) maxc = cl;
  }
  if (nClasses <= 0) nClasses = maxc + 1;
  if (maxc >= nClasses) return fail(c, GTX_E_RANGE, "gtx_set_refs: class id >= n_classes");
  if (nClasses < 1) nClasses = 1;

  // valid regions only take part (genomic_intervals.cpp:5659: start>stop or stop<=0 is skipped)
  std::vector<u64> keyE, keyS;                   // (class, biased coordinate, ordinal) packed for one sort each
  std::vector<int32_t> ord;
  ord.reserve(m);
  const bool keepZero = (flags & GTX_REFS_KEEP_ZERO_LENGTH) != 0;
  for (int64_t k = 0; k < m; k++) {
    int32_t s = tri[3 * k + 1], e = tri[3 * k + 2];
    const bool take = tri[3 * k] >= 0 && (keepZero ? (int64_t)s <= (int64_t)e + 1 : !(s > e || e <= 0));
    if (take) ord.push_back((int32_t)k);
  }
  const int64_t nv = (int64_t)ord.size();
  struct Item { int32_t cls; int32_t val; int32_t k; };
  std::vector<Item> itE(nv), itS(nv);
  for (int64_t i = 0; i < nv; i++) {
    int32_t k = ord[i];
    itE[i] = {tri[3 * (int64_t)k], tri[3 * (int64_t)k + 2], k};
    itS[i] = {tri[3 * (int64_t)k], tri[3 * (int64_t)k + 1], k};
  }
  auto cmp = [](const Item &a, const Item &b) { return a.cls != b.cls ? a.cls < b.cls : (a.val != b.val ? a.val < b.val : a.k < b.k); };
  if (nv > (1 << 16)) {                                      // the two orders are independent: sort them side by side
    std::thread other([&] { std::sort(itS.begin(), itS.end(), cmp); });
    std::sort(itE.begin(), itE.end(), cmp);
    other.join();
  } else {
    std::sort(itE.begin(), itE.end(), cmp);
    std::sort(itS.begin(), itS.end(), cmp);
  }

  std::vector<int32_t> sortedE(nv + 1), sortedS(nv + 1), seg(nClasses + 1, 0), posE(m > 0 ? m : 1, -1), posS(m > 0 ? m : 1, -1), classBase(m > 0 ? m : 1, -1);
  for (int64_t i = 0; i < nv; i++) seg[itE[i].cls + 1]++;
  for (int cl = 0; cl < nClasses; cl++) seg[cl + 1] += seg[cl];
  for (int64_t i = 0; i < nv; i++) {
    sortedE[i] = itE[i].val; posE[itE[i].k] = (int32_t)(i + itE[i].cls);
    sortedS[i] = itS[i].val; posS[itS[i].k] = (int32_t)(i + itS[i].cls);
    classBase[itE[i].k] = seg[itE[i].cls] + itE[i].cls - 1;
  }

  // everything made from the old set goes before the new set is made (never both at once)
  c->nRefs = -1;
  c->ix = {}; c->cv = {}; c->rx = {}; c->share = {};
  c->covDirty = false; c->pairUsed = false;
  const int64_t histLen = nv + nClasses;
  HIPCHK(c, c->ix.sortedE.alloc(nv + 1));
  HIPCHK(c, c->ix.sortedS.alloc(nv + 1));
  HIPCHK(c, c->ix.segStart.alloc(nClasses + 1));
  HIPCHK(c, c->ix.posE.alloc(m + 1));
  HIPCHK(c, c->ix.posS.alloc(m + 1));
  HIPCHK(c, c->ix.classBase.alloc(m + 1));
  { int rc = make_hist_set(c, c->ix.hist, histLen); if (rc) return rc; }
  c->histDirty = false; c->tileSumsValid = true;
  HIPCHK(c, hipMemcpy(c->ix.sortedE.get(), sortedE.data(), sizeof(int32_t) * nv, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->ix.sortedS.get(), sortedS.data(), sizeof(int32_t) * nv, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->ix.segStart.get(), seg.data(), sizeof(int32_t) * (nClasses + 1), hipMemcpyHostToDevice));
  {
    c->ix.sampShift = gtx::search_sample_shift(nv);
    c->ix.nSamp = (int)((nv + (1ll << c->ix.sampShift) - 1) >> c->ix.sampShift);
    std::vector<int32_t> sampE(c->ix.nSamp + 1), sampS(c->ix.nSamp + 1);
    for (int i = 0; i < c->ix.nSamp; i++) { sampE[i] = sortedE[(int64_t)i << c->ix.sampShift]; sampS[i] = sortedS[(int64_t)i << c->ix.sampShift]; }
    HIPCHK(c, upload(c->ix.sampE, sampE.data(), sampE.size()));
    HIPCHK(c, upload(c->ix.sampS, sampS.data(), sampS.size()));
    const int64_t nTop = (nv + 255) >> 8;
    std::vector<int32_t> topE(nTop + 1), topS(nTop + 1);
    for (int64_t i = 0; i < nTop; i++) { topE[i] = sortedE[i << 8]; topS[i] = sortedS[i << 8]; }
    HIPCHK(c, upload(c->ix.topE, topE.data(), topE.size()));
    HIPCHK(c, upload(c->ix.topS, topS.data(), topS.size()));
  }
  { int rc = make_place_table(c, seg, sortedE, sortedS, nClasses, nv, c->ix.place); if (rc) return rc; }
  {
    // bucket table of the unsorted path: cuts of the ends array every bucket_e_size() boundaries, never across classes
    const int kE = gtx::bucket_e_size(), kS = gtx::bucket_s_size();
    BucketCuts k;
    k.clsStart.assign(nClasses + 1, 0);
    for (int cl = 0; cl < nClasses; cl++) {
      k.clsStart[cl] = (int32_t)k.posHi.size();
      const int32_t s0 = seg[cl], s1 = seg[cl + 1];
      for (int32_t e0 = s0; e0 < s1; e0 += kE) {
        const int32_t e1 = std::min<int64_t>((int64_t)e0 + kE, s1);
        k.posHi.push_back(e1 == s1 ? INT32_MAX : sortedE[e1 - 1]);
        k.eLo.push_back(e0); k.eHi.push_back(e1); k.cls.push_back(cl);
        // a read of this bucket starts above E[e0-1], so it ends at or above it: ranks in the starts array begin here
        const int32_t lo = e0 == s0 ? s0 : (int32_t)(std::upper_bound(sortedS.begin() + s0, sortedS.begin() + s1, sortedE[e0 - 1]) - sortedS.begin());
        k.sLo.push_back(lo); k.sHi.push_back((int32_t)std::min<int64_t>((int64_t)lo + kS, s1));
      }
    }
    k.clsStart[nClasses] = (int32_t)k.posHi.size();
    if (k.posHi.size() <= 8192 && nClasses <= 2048) {            // (else certainly too many for the LDS tables of the scatter kernel)
      int rc = build_bucket_tables(c, c->ix.bkt, k, nClasses); if (rc) return rc;
    }
  }
  if (m > 0) {
    HIPCHK(c, hipMemcpy(c->ix.posE.get(), posE.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ix.posS.get(), posS.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ix.classBase.get(), classBase.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
  }
  c->h_refS.resize(m > 0 ? m : 1); c->h_refE.resize(m > 0 ? m : 1); c->h_refC.resize(m > 0 ? m : 1);
  for (int64_t k = 0; k < m; k++) { c->h_refC[k] = tri[3 * k]; c->h_refS[k] = tri[3 * k + 1]; c->h_refE[k] = tri[3 * k + 2]; }
  c->mergeRefs = keepZero;
  if (keepZero) {
    std::vector<int4> sp; std::vector<int32_t> spIdx;
    for (int64_t k = 0; k < m; k++)
      if (tri[3 * k] >= 0 && (int64_t)tri[3 * k + 1] > (int64_t)tri[3 * k + 2] + 1) { sp.push_back(make_int4(tri[3 * k], tri[3 * k + 1], tri[3 * k + 2], 0)); spIdx.push_back((int32_t)k); }
    c->rx.nSpecial = (int)sp.size();
    if (c->rx.nSpecial) {
      HIPCHK(c, upload(c->rx.specialRefs, sp.data(), sp.size()));
      HIPCHK(c, upload(c->rx.specialIdx, spIdx.data(), spIdx.size()));
      HIPCHK(c, c->rx.specialOut.alloc(sp.size()));
      HIPCHK(c, hipMemset(c->rx.specialOut.get(), 0, sizeof(u64) * sp.size()));
    }
  }
  c->nRefs = m; c->nValid = nv; c->nClasses = nClasses; c->histLen = histLen;
  c->h_seg = seg;
  return GTX_OK;
}

// ---------------------------------------------------------------------------------------------
// count
// ---------------------------------------------------------------------------------------------
#ifdef GTX_WAVE_TRACE
// diagnostic build (make trace -> libgtx_trace.so, scripts/wave_trace.py): per-wave time stamps of the streaming count kernel
static constexpr size_t kTraceWaves = 1u << 20;
static unsigned long long *g_trace = nullptr;
static unsigned long long *gtx_debug_trace_buffer()
{
  if (!g_trace && hipMalloc(&g_trace, kTraceWaves * 32) == hipSuccess) (void)hipMemset(g_trace, 0, kTraceWaves * 32);
  return g_trace;
}
extern "C" int gtx_debug_trace_read(unsigned long long *out, long long nWaves)
{
  if (!g_trace || nWaves > (long long)kTraceWaves) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  if (hipMemcpy(out, g_trace, (size_t)nWaves * 32, hipMemcpyDeviceToHost) != hipSuccess) return -3;
  return hipMemset(g_trace, 0, kTraceWaves * 32) == hipSuccess ? 0 : -4;      // (the next launch may have fewer waves)
}
#endif

} // extern "C"

// the count kernels' arguments over histogram set h.  hist32: the call is ONE launch of the streaming kernel over unweighted reads
// (a *_device call): 32-bit histogram slots (CountArgs::hist32); the caller hands the same flag to launch_finalize
gtx::CountArgs count_args(gtx_ctx *c, const HistSet &h, uint32_t flags, int64_t nReads, int64_t indexBase, CountCall who, bool hist32)
{
  gtx::CountArgs a;
  a.indexBase = indexBase;
  const gtx::RouteKnobs &knobs = gtx::route_knobs();
  a.hist32 = gtx::hist32_slots(hist32, nReads, knobs);
  a.owned = who != COUNT_ANY && c->share.on ? c->share.owned.get() : nullptr;
  a.sortedE = c->ix.sortedE.get(); a.sortedS = c->ix.sortedS.get(); a.segStart = c->ix.segStart.get();
  a.histA = h.histA.get(); a.histB = h.histB.get(); a.partA = h.partA.get(); a.partB = h.partB.get(); a.info = c->d_info.get() + c->infoCur;
  a.nClasses = c->nClasses;
  if (!gtx::keeps_tile_sums(c->histLen, nReads, knobs)) { a.partA = nullptr; a.partB = nullptr; c->tileSumsValid = false; }
  const int r = 4;                                // reads per lane per step of the streaming kernel
  a.chunksPerWave = gtx::count_chunks_per_wave(nReads, c->waveSlots, c->chunksPerWave);
  a.sched = gtx::span_schedule((nReads + 63) >> 6, a.chunksPerWave, r, c->waveSlots);
  a.checkSorted = (flags & GTX_CHECK_SORTED) ? 1 : 0; a.sortClassShift = 0;
  a.zeroLenOk = (flags & GTX_ZERO_LENGTH_OK) ? 1 : 0;
  const bool merge = (flags & GTX_ZERO_LENGTH_OK) && c->mergeRefs && c->side.get();       // full sorted-merge semantics (see merge_prepare)
  a.side = merge ? c->side.get() : nullptr; a.sideCount = merge ? c->sideCount.get() : nullptr; a.sideCap = c->sideCap; a.coverRule = 0; a.keyCenter = 0;
  a.sampE = c->ix.sampE.get(); a.sampS = c->ix.sampS.get(); a.sampShift = c->ix.sampShift; a.nSamp = c->ix.nSamp;
  a.topE = c->ix.topE.get(); a.topS = c->ix.topS.get();
  a.place = c->ix.place.view();
  // (a group member's async call streams the reads of ITS classes only: their density is against its own regions, not the whole set's)
  a.flip = gtx::flip_walk(who == COUNT_SHARE_ASYNC && c->share.on ? std::min<int64_t>(c->nValid, c->share.nRegions) : c->nValid, nReads, knobs);
#ifdef GTX_WAVE_TRACE
  a.trace = gtx_debug_trace_buffer();
#endif
  return a;
}

// scratch of the partition path for a call of plan p (grown, never shrunk), and the views the kernels take
static int bucket_scratch(gtx_ctx *c, const gtx::BucketPlan &p, int nB, gtx::BucketWork *w)
{
  if (p.pairs > c->bktReads.cap || !c->bktDir) {                     // (bktDir made last: there, all three are)
    c->bktReads.reset(); c->bktWeights.reset(); c->bktDir.reset();
    HIPCHK(c, c->bktReads.alloc(p.pairs));
    HIPCHK(c, c->bktWeights.alloc(p.pairs));
    HIPCHK(c, c->bktDir.alloc(2 * p.chunks));                         // directory | list
  }
  HIPCHK(c, c->bktCnt.reserve(p.matrix + p.blocks + (size_t)nB + 1));  // chunkCount | arenaUsed | rowOff
  w->tmpReads = c->bktReads.get(); w->tmpWeights = c->bktWeights.get(); w->arenaPairs = (unsigned)p.arenaPairs;
  w->dir = c->bktDir.get(); w->list = c->bktDir.get() + c->bktReads.cap / 64; w->chunkCount = c->bktCnt.get(); w->arenaUsed = c->bktCnt.get() + p.matrix; w->rowOff = w->arenaUsed + p.blocks;
  return GTX_OK;
}

// THE decision for the partition path, made once per batch of reads in no particular order: tables t are there, the batch is worth
// partitioning and its plan fits 32-bit pair indices.  On yes the scratch is ready (*p, *w).
int partition_plan(gtx_ctx *c, const BucketTables &t, int64_t n, int nClasses, bool weighted, gtx::BucketPlan *p, gtx::BucketWork *w, bool *yes)
{
  *yes = false;
  if (t.nB == 0 || !gtx::partition_worth(n, c->bucketMinReads)) return GTX_OK;
  *p = gtx::bucket_plan(n, nClasses, t.nB, t.nCells, weighted);
  if (!(p->pairs < (1ull << 32))) return GTX_OK;
  *yes = true;
  return bucket_scratch(c, *p, t.nB, w);
}

// reads in no particular order: bucket partition + LDS counting for large batches, per-read search kernel otherwise
int launch_unsorted(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, const gtx::CountArgs &a)
{
  gtx::BucketPlan p; gtx::BucketWork w; bool part;
  { int rc = partition_plan(c, c->ix.bkt, n, a.nClasses, d_weights != nullptr, &p, &w, &part); if (rc) return rc; }
  if (part) HIPCHK(c, gtx::launch_count_bucketed(d_reads, d_weights, n, a, c->ix.bkt.view(), w, p, c->stream));
  else HIPCHK(c, gtx::launch_count(d_reads, d_weights, n, a, false, c->stream));
  return GTX_OK;
}

// Full sorted-merge semantics (GTX_ZERO_LENGTH_OK on a reference set given with GTX_REFS_KEEP_ZERO_LENGTH): intervals with
// start > end + 1 take part by the merge's two comparisons (gtx_special.hip).  Buffers are made on first use.
int ref_columns(gtx_ctx *c)
{
  if (!c->rx.refE) {
    HIPCHK(c, c->rx.refS.alloc(c->nRefs + 1));
    HIPCHK(c, c->rx.refE.alloc(c->nRefs + 1));
    if (c->nRefs > 0) {
      HIPCHK(c, hipMemcpy(c->rx.refS.get(), c->h_refS.data(), sizeof(int32_t) * c->nRefs, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(c->rx.refE.get(), c->h_refE.data(), sizeof(int32_t) * c->nRefs, hipMemcpyHostToDevice));
    }
  }
  return GTX_OK;
}

int merge_prepare(gtx_ctx *c, uint32_t flags, int mode)
{
  if (!(flags & GTX_ZERO_LENGTH_OK) || !c->mergeRefs) return GTX_OK;
  if (!c->sideCount) {
    HIPCHK(c, c->side.alloc((size_t)c->sideCap));
    HIPCHK(c, c->sideCount.alloc(1));
    HIPCHK(c, hipMemset(c->sideCount.get(), 0, sizeof(unsigned)));
  }
  if (!c->rx.refC) {
    int rc = ref_columns(c); if (rc) return rc;
    HIPCHK(c, c->rx.refC.alloc(c->nRefs + 1));
    if (c->nRefs > 0) HIPCHK(c, hipMemcpy(c->rx.refC.get(), c->h_refC.data(), sizeof(int32_t) * c->nRefs, hipMemcpyHostToDevice));
  }
  c->sideUsed = true; c->specialMode = mode;
  return GTX_OK;
}

// after the count kernels of one batch, multi-interval index regions (gtx_set_ref_blocks): a read with one interval that lies in
// a gap of such a region was counted on the region's envelope -- off again
int pairs_batch(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n)
{
  if (c->rx.pairMulti.n > 0) {
    HIPCHK(c, gtx::launch_pair_miss(d_reads, d_weights, n, c->rx.pairMulti.ix, gtx::RegionBlocks{c->rx.blkOf.get(), c->rx.blkIv.get()}, c->rx.pairAcc.get() + c->nRefs, c->stream));
    c->pairUsed = true;
  }
  return GTX_OK;
}

// after the kernels of one batch: the batch against the inverted reference regions
int merge_batch(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n)
{
  if (c->sideUsed && c->rx.nSpecial) HIPCHK(c, gtx::launch_special_refs(d_reads, d_weights, n, c->rx.specialRefs.get(), c->rx.nSpecial, c->specialMode, c->rx.specialOut.get(), c->stream));
  return GTX_OK;
}

// after the gather: the inverted reads against the other regions, then the inverted regions' sums into their places
int merge_end(gtx_ctx *c, void *d_out)
{
  if (c->pairUsed) {
    c->pairUsed = false;
    HIPCHK(c, gtx::launch_pair_apply((u64 *)d_out, c->rx.pairAcc.get(), c->rx.pairAcc.get() + c->nRefs, c->nRefs, c->stream));
  }
  if (!c->sideUsed) return GTX_OK;
  c->sideUsed = false;
  HIPCHK(c, gtx::launch_side_reads(c->rx.refC.get(), c->rx.refS.get(), c->rx.refE.get(), c->nRefs, c->side.get(), c->sideCount.get(), c->sideCap, c->specialMode, (u64 *)d_out,
                                   c->d_info.get() + c->infoCur, c->stream));
  HIPCHK(c, gtx::launch_special_scatter(c->rx.specialIdx.get(), c->rx.specialOut.get(), c->rx.nSpecial, (u64 *)d_out, c->sideCount.get(), c->stream));
  return GTX_OK;
}

extern "C" {

// begin: zero histograms + info; accumulate: one kernel per resident batch; end: prefix + gather
static int count_begin(gtx_ctx *c)
{
  if (c->histDirty) {                             // only after an abandoned call
    HistSet &h = c->ix.hist;
    for (DevBuf<u64> *b : {&h.histA, &h.histB, &h.partA, &h.partB, &h.totals}) HIPCHK(c, hipMemsetAsync(b->get(), 0, sizeof(u64) * b->cap, c->stream));
  }
  // the info block is shared by count and coverage calls: an abandoned call of either kind leaves counts in it
  if (c->histDirty || c->covDirty) HIPCHK(c, hipMemcpyAsync(c->d_info.get() + c->infoCur, &c->h_info.get()[1], sizeof(gtx::DevInfo), hipMemcpyHostToDevice, c->stream));
  if ((c->histDirty || c->covDirty) && c->sideCount.get()) {            // an abandoned call may have left inverted reads / sums behind
    HIPCHK(c, hipMemsetAsync(c->sideCount.get(), 0, sizeof(unsigned), c->stream));
    if (c->rx.nSpecial) HIPCHK(c, hipMemsetAsync(c->rx.specialOut.get(), 0, sizeof(u64) * c->rx.nSpecial, c->stream));
  }
  if (c->histDirty && c->rx.pairAcc.get()) HIPCHK(c, hipMemsetAsync(c->rx.pairAcc.get(), 0, sizeof(u64) * 2 * (size_t)std::max<int64_t>(c->nRefs, 1), c->stream));
  c->sideUsed = false; c->pairUsed = false;
  c->histDirty = true; c->tileSumsValid = true;
  c->ix.lastShareInfo = nullptr;
  return GTX_OK;
}

// the finalize step of a count call over set h on stream s: counts of info, infoNext reset for the call after; fs: a group member's
// classes only
static int finalize_set(gtx_ctx *c, HistSet &h, bool sumsValid, u64 *d_hits, gtx::DevInfo *info, gtx::DevInfo *infoNext, hipStream_t s,
                        const gtx::FinalizeShare *fs, bool hist32)
{
  if (++h.epoch == 0) { HIPCHK(c, hipMemsetAsync(h.flags.get(), 0, sizeof(unsigned) * h.flags.cap, s)); h.epoch = 1; h.draws = 0; }   // (after 2^32 calls: the flags start over)
  gtx::FinalizeArgs a = h.view(c->histLen);
  a.tileSumsValid = sumsValid; a.localMaxTiles = c->localMaxTiles; a.posE = c->ix.posE.get(); a.posS = c->ix.posS.get(); a.classBase = c->ix.classBase.get();
  a.m = c->nRefs; a.hits = d_hits; a.info = info; a.nextInfo = infoNext; a.share = fs; a.hist32 = hist32;
  gtx::FinalizeRoute took;
  HIPCHK(c, gtx::launch_finalize(a, s, &took));
  // the launch is in the stream: the chained kernel has drawn a ticket per tile it ran, the local gather has zeroed the other turn's totals
  if (took == gtx::FIN_CHAINED) h.draws += (unsigned long long)(fs ? fs->nTiles : gtx::scan_tiles(c->histLen));
  if (took == gtx::FIN_LOCAL) h.totalsTurn ^= 1;
  return GTX_OK;
}

// share: the context is a group member -- finalize its classes only, d_hits receives its regions in the group's compact order
static int count_end(gtx_ctx *c, void *d_hits, bool share = false, bool scatter = false, bool hist32 = false)
{
  const gtx::FinalizeShare fs = {c->share.tiles.get(), c->share.nTiles, c->share.regions.get(), c->share.nRegions, scatter};
  int rc = finalize_set(c, c->ix.hist, c->tileSumsValid, (u64 *)d_hits, c->d_info.get() + c->infoCur, c->d_info.get() + (c->infoCur ^ 1), c->stream,
                        share ? &fs : nullptr, hist32);
  if (rc) return rc;
  rc = merge_end(c, d_hits); if (rc) return rc;
  c->histDirty = false;
  c->infoCur ^= 1;                                // the block just used stays readable until the call after next
  return GTX_OK;
}

int gtx_count_device(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, uint32_t flags, void *d_hits)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_count_device: gtx_set_refs has not been called");
  if (n < 0 || (n > 0 && !d_reads) || (c->nRefs > 0 && !d_hits)) return fail(c, GTX_E_ARG, "gtx_count_device: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = count_begin(c); if (rc) return rc;
  prof_begin(c);
  HIPCHK(c, prof_mark(c, 1, c->stream));
  rc = merge_prepare(c, flags, 0); if (rc) return rc;
  // GTX_CHECK_SORTED is answered by the streaming kernel (exact for any order; only it looks at the order of the reads)
  const bool streaming = (flags & (GTX_READS_SORTED | GTX_CHECK_SORTED)) != 0;
  if (!streaming) c->tileSumsValid = false;
  bool h32 = false;
  if (streaming) {
    const gtx::CountArgs a = count_args(c, c->ix.hist, flags, n, 0, COUNT_ANY, d_weights == nullptr);
    h32 = a.hist32 != 0 && n > 0;
    HIPCHK(c, gtx::launch_count(d_reads, d_weights, n, a, true, c->stream));
  }
  else { rc = launch_unsorted(c, d_reads, d_weights, n, count_args(c, c->ix.hist, flags, n)); if (rc) return rc; }
  rc = merge_batch(c, d_reads, d_weights, n); if (rc) return rc;
  rc = pairs_batch(c, d_reads, d_weights, n); if (rc) return rc;
  HIPCHK(c, prof_mark(c, 2, c->stream));
  rc = count_end(c, d_hits, false, false, h32); if (rc) return rc;
  HIPCHK(c, prof_end(c, c->stream));
  return GTX_OK;
}

static void info_out(const gtx::DevInfo &d, gtx_count_info *o, int64_t base)
{
  o->first_unsorted = d.first_unsorted == INT64_MAX ? -1 : d.first_unsorted + base;
  o->n_no_class = d.n_no_class; o->n_degenerate = d.n_degenerate;
  o->first_degenerate = d.first_degenerate == INT64_MAX ? -1 : d.first_degenerate + base;
  o->n_unplaced = d.n_unplaced;
}

// a kernel of the call gave up a bounded wait (DevInfo::fault): its result vector is void
static int fault_check(gtx_ctx *c, const gtx::DevInfo &d)
{
  return d.fault ? fail(c, GTX_E_HIP, "the finalize step gave up waiting for a tile sum (finalize_scan_chained_kernel): the result of this call is void; GTX_CHAINED_SCAN=0 takes the two-launch finalize") : GTX_OK;
}

int gtx_last_info(gtx_ctx *c, gtx_count_info *info)
{
  if (!c || !info) return GTX_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(&c->h_info.get()[0], c->d_info.get() + (c->infoCur ^ 1), sizeof(gtx::DevInfo), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  info_out(c->h_info.get()[0], info, 0);
  return fault_check(c, c->h_info.get()[0]);
}

} // extern "C" (templates below)

// ---------------------------------------------------------------------------------------------
// host buffers -> device, double-buffered
// ---------------------------------------------------------------------------------------------
// A batch of the caller's reads travels: [pageable memory -> pinned slot (host threads)] -> device slot (DMA on the copy
// stream) -> kernels (the context's stream).  Two slots of each kind alternate, so the copy of batch i+1 -- host part and
// DMA -- runs under the kernels of batch i; the only host waits are for a slot to come free.  Memory the caller obtained
// from gtx_host_alloc (or any other page-locked memory HIP knows) skips the pinned slot: the DMA reads it directly.
bool is_pinned(const void *p)
{
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

void parallel_copy(char *dst, const char *src, size_t bytes, int threads)
{
  const int T = (int)std::min<size_t>((size_t)threads, bytes / (4u << 20) + 1);
  if (T <= 1) { memcpy(dst, src, bytes); return; }
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back([=] { const size_t b0 = bytes * (size_t)t / T, b1 = bytes * (size_t)(t + 1) / T; memcpy(dst + b0, src + b0, b1 - b0); });
  memcpy(dst, src, bytes / T);
  for (auto &x : th) x.join();
}

int stage_reserve(gtx_ctx *c, size_t nReads, bool weights, bool pinnedSlots)
{
  const size_t bytes = nReads * 12, nW = weights ? nReads : 0, pinBytes = pinnedSlots ? nReads * 16 : 0;
  bool grows = false;
  for (int k = 0; k < 2; k++) grows |= bytes > c->stage.dev[k].cap || nW > c->stage.devW[k].cap || pinBytes > c->stage.pin[k].cap;
  if (grows) {
    // growing: nothing may still be in flight on the old buffers
    HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage.slotBusy[0] = c->stage.slotBusy[1] = false;
  }
  for (int k = 0; k < 2; k++) HIPCHK(c, c->stage.dev[k].reserve(bytes));
  for (int k = 0; k < 2; k++) HIPCHK(c, c->stage.devW[k].reserve(nW));
  for (int k = 0; k < 2; k++) HIPCHK(c, c->stage.pin[k].reserve(pinBytes));
  return GTX_OK;
}

int ensure_out(gtx_ctx *c, size_t n)
{
  HIPCHK(c, c->out.reserve(n, n + 1));
  return GTX_OK;
}

extern "C" {

// Host buffers: the reads are streamed through the device in batches (the histograms simply keep
// accumulating across batches), so N is bounded by host memory only -- the analogue of the
// reference never holding the query set in memory (genomic_intervals.cpp:3855-3861).
int gtx_count_begin(gtx_ctx *c)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_count_begin: gtx_set_refs has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = count_begin(c); if (rc) return rc;
  c->streamSeen = 0; c->streamOpen = true; c->streamLast[0] = c->streamLast[1] = INT32_MIN; c->seamUnsorted = INT64_MAX;
  return GTX_OK;
}

int gtx_count_add(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, uint32_t flags)
{
  if (!c) return GTX_E_ARG;
  if (!c->streamOpen) return fail(c, GTX_E_STATE, "gtx_count_add: gtx_count_begin has not been called");
  if (n < 0 || (n > 0 && !reads)) return fail(c, GTX_E_ARG, "gtx_count_add: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  const bool streaming = (flags & (GTX_READS_SORTED | GTX_CHECK_SORTED)) != 0;
  if ((flags & GTX_CHECK_SORTED) && n > 0) {
    // order across the seams between batches (inside a batch the kernel checks): host-side, two reads per seam
    const int64_t batch = c->batchReads;
    for (int64_t off = 0; off < n; off += batch) {
      const int32_t *q = reads + 3 * off;
      const int32_t pc = off ? q[-3] : c->streamLast[0], ps = off ? q[-2] : c->streamLast[1];
      if ((c->streamSeen + off) > 0 && (q[0] < pc || (q[0] == pc && q[1] < ps)) && c->seamUnsorted == INT64_MAX) c->seamUnsorted = c->streamSeen + off;
    }
  }
  if (n > 0) { c->streamLast[0] = reads[3 * (n - 1)]; c->streamLast[1] = reads[3 * (n - 1) + 1]; }
  const int64_t seen = c->streamSeen;
  int rc = merge_prepare(c, flags, 0); if (rc) return rc;
  rc = stage_batches(c, reads, weights, n, [&](const void *dR, const int *dW, int64_t cnt, int64_t off) -> int {
    // indices in the info block are positions in the whole stream (indexBase); the block accumulates over the batches
    if (!streaming) c->tileSumsValid = false;
    if (streaming) HIPCHK(c, gtx::launch_count(dR, dW, cnt, count_args(c, c->ix.hist, flags, cnt, seen + off), true, c->stream));
    else { int rcu = launch_unsorted(c, dR, dW, cnt, count_args(c, c->ix.hist, flags, cnt, seen + off)); if (rcu) return rcu; }
    { int rcp = pairs_batch(c, dR, dW, cnt); if (rcp) return rcp; }
    return merge_batch(c, dR, dW, cnt);
  });
  if (rc) return rc;
  c->streamSeen += n;
  return GTX_OK;
}

// closes the open stream call: finalize into the context's own output vector in HBM (enqueued, not waited for)
// share != 0 (a group member with gtxi_set_share): only its classes are finalized, *d_out = its piece of the group's compact vector
int gtxi_count_finish(gtx_ctx *c, void **d_out, int share)
{
  if (!c->streamOpen) return fail(c, GTX_E_STATE, "gtx_count_end: gtx_count_begin has not been called");
  if (share && !c->share.on) return fail(c, GTX_E_STATE, "gtxi_count_finish: no share set");
  if (share && (c->rx.refBlocks || c->pairUsed)) return fail(c, GTX_E_STATE, "gtxi_count_finish: multi-interval regions are finalized over the whole vector");
  HIPCHK(c, hipSetDevice(c->device));
  c->streamOpen = false;
  int rc = ensure_out(c, (size_t)c->nRefs); if (rc) return rc;
  u64 *dst = share ? c->out.get() + c->share.offset : c->out.get();
  rc = count_end(c, dst, share != 0); if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(&c->h_info.get()[0], c->d_info.get() + (c->infoCur ^ 1), sizeof(gtx::DevInfo), hipMemcpyDeviceToHost, c->stream));
  *d_out = dst;
  return GTX_OK;
}

// after gtxi_*_finish and a wait for the stream: what the call observed
void gtxi_fetch_info(gtx_ctx *c, gtx_count_info *info)
{
  info_out(c->h_info.get()[0], info, 0);
  if (c->seamUnsorted != INT64_MAX && (info->first_unsorted < 0 || c->seamUnsorted < info->first_unsorted)) info->first_unsorted = c->seamUnsorted;
}

int gtx_count_end(gtx_ctx *c, uint64_t *hits, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->streamOpen && c->nRefs > 0 && !hits) return fail(c, GTX_E_ARG, "gtx_count_end: null output");
  void *d = nullptr;
  int rc = gtxi_count_finish(c, &d, 0); if (rc) return rc;
  if (c->nRefs > 0) HIPCHK(c, hipMemcpyAsync(hits, d, sizeof(u64) * c->nRefs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
  if (info) gtxi_fetch_info(c, info);
  return fault_check(c, c->h_info.get()[0]);
}

int gtx_count(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, uint32_t flags, uint64_t *hits, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_count: gtx_set_refs has not been called");
  if (n < 0 || (n > 0 && !reads) || (c->nRefs > 0 && !hits)) return fail(c, GTX_E_ARG, "gtx_count: bad argument");
  int rc = gtx_count_begin(c); if (rc) return rc;
  rc = gtx_count_add(c, reads, weights, n, flags); if (rc) { c->streamOpen = false; return rc; }
  return gtx_count_end(c, hits, info);
}

// ---------------------------------------------------------------------------------------------
// count without -gaps over multi-interval regions (gtx_pairs.hip)
// ---------------------------------------------------------------------------------------------
} // extern "C"

static int pair_acc(gtx_ctx *c)
{
  if (c->rx.pairAcc) return GTX_OK;
  const size_t n = 2 * (size_t)std::max<int64_t>(c->nRefs, 1);
  HIPCHK(c, c->rx.pairAcc.alloc(n));
  HIPCHK(c, hipMemset(c->rx.pairAcc.get(), 0, sizeof(u64) * n));
  return GTX_OK;
}

// {start, stop} lists as the kernels need them: starts and stops both non-decreasing (sorted, disjoint intervals are)
bool blocks_monotone(const int32_t *b, int64_t cnt)
{
  for (int64_t j = 1; j < cnt; j++) if (b[2 * j] < b[2 * j - 2] || b[2 * j + 1] < b[2 * j - 1]) return false;
  return true;
}

// the reference regions' interval lists as the kernels take them (none: every region is its envelope)
gtx::RegionBlocks ref_blocks(const gtx_ctx *c) { return gtx::RegionBlocks{c->rx.refBlocks ? c->rx.blkOf.get() : nullptr, c->rx.blkIv.get()}; }

extern "C" {

int gtx_set_ref_blocks(gtx_ctx *c, const int64_t *first, const int32_t *blocks)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_set_ref_blocks: gtx_set_refs has not been called");
  if (c->streamOpen || c->covOpen) return fail(c, GTX_E_STATE, "gtx_set_ref_blocks: a call is open");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rx.pairMulti = {}; c->rx.pairAll = {}; c->rx.blkOf.reset(); c->rx.blkIv.reset(); c->rx.refBlocks = false; c->rx.joinMono = -1; c->rx.offRef.reset();
  if (!first) return GTX_OK;                                   // back to single-interval regions
  const int64_t m = c->nRefs;
  if (first[0] != 0) return fail(c, GTX_E_ARG, "gtx_set_ref_blocks: first[0] must be 0");
  if (first[m] >= INT32_MAX || (first[m] > 0 && !blocks)) return fail(c, GTX_E_ARG, "gtx_set_ref_blocks: bad argument");
  std::vector<int2> blkOf((size_t)std::max<int64_t>(m, 1), make_int2(0, 0)), iv;
  for (int64_t k = 0; k < m; k++) {
    const int64_t cnt = first[k + 1] - first[k];
    if (cnt < 1) return fail(c, GTX_E_ARG, "gtx_set_ref_blocks: every region has at least one interval");
    const int32_t *b = blocks + 2 * first[k];
    if (c->h_refC[k] >= 0 && (b[0] != c->h_refS[k] || b[2 * cnt - 1] != c->h_refE[k]))
      return fail(c, GTX_E_ARG, "gtx_set_ref_blocks: a region's triple must be its envelope (first interval's start, last interval's stop)");
    if (cnt == 1 || c->h_refC[k] < 0) continue;
    if (!blocks_monotone(b, cnt)) return fail(c, GTX_E_RANGE, "gtx_set_ref_blocks: the intervals of a region must be sorted (starts and stops non-decreasing)");
    blkOf[k] = make_int2((int)iv.size(), (int)cnt);
    for (int64_t j = 0; j < cnt; j++) iv.push_back(make_int2(b[2 * j], b[2 * j + 1]));
  }
  if (iv.empty()) return GTX_OK;                               // no multi-interval region: nothing to correct
  HIPCHK(c, upload(c->rx.blkOf, blkOf.data(), blkOf.size()));
  HIPCHK(c, upload(c->rx.blkIv, iv.data(), iv.size()));
  int rc = build_pair_index(c, &c->rx.pairMulti, [&](int64_t k) { return blkOf[k].y > 0; }); if (rc) return rc;
  rc = pair_acc(c); if (rc) return rc;
  c->rx.refBlocks = true;
  return GTX_OK;
}

int gtx_count_add_regions(gtx_ctx *c, const int32_t *env, const int32_t *weights, const int64_t *first, const int32_t *blocks, int64_t n)
{
  if (!c) return GTX_E_ARG;
  if (!c->streamOpen) return fail(c, GTX_E_STATE, "gtx_count_add_regions: gtx_count_begin has not been called");
  if (n < 0 || (n > 0 && (!env || !first || !blocks))) return fail(c, GTX_E_ARG, "gtx_count_add_regions: bad argument");
  if (n == 0) return GTX_OK;
  if (first[0] != 0 || first[n] >= INT32_MAX) return fail(c, GTX_E_ARG, "gtx_count_add_regions: bad interval lists");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int4> q((size_t)n); std::vector<int2> qb((size_t)n), iv((size_t)first[n]);
  for (int64_t i = 0; i < n; i++) {
    const int64_t cnt = first[i + 1] - first[i];
    if (cnt < 1) return fail(c, GTX_E_ARG, "gtx_count_add_regions: every region has at least one interval");
    const int32_t *b = blocks + 2 * first[i];
    if (b[0] != env[3 * i + 1] || b[2 * cnt - 1] != env[3 * i + 2]) return fail(c, GTX_E_ARG, "gtx_count_add_regions: a region's triple must be its envelope");
    if (!blocks_monotone(b, cnt)) return fail(c, GTX_E_RANGE, "gtx_count_add_regions: the intervals of a region must be sorted (starts and stops non-decreasing)");
    q[i] = make_int4(env[3 * i], env[3 * i + 1], env[3 * i + 2], weights ? weights[i] : 1);
    qb[i] = make_int2((int)first[i], (int)cnt);
    for (int64_t j = 0; j < cnt; j++) iv[first[i] + j] = make_int2(b[2 * j], b[2 * j + 1]);
  }
  if (!c->rx.pairAll.built) { int rc = build_pair_index(c, &c->rx.pairAll, [](int64_t) { return true; }); if (rc) return rc; }
  { int rc = pair_acc(c); if (rc) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->stream));                  // (the kernel of the previous call may still read the query buffers)
  if ((size_t)n > c->pairQBlk.cap) { c->pairQ.reset(); c->pairQBlk.reset(); HIPCHK(c, c->pairQ.alloc((size_t)n)); HIPCHK(c, c->pairQBlk.alloc((size_t)n)); }
  HIPCHK(c, c->pairQIv.reserve(iv.size()));
  HIPCHK(c, hipMemcpy(c->pairQ.get(), q.data(), sizeof(int4) * (size_t)n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->pairQBlk.get(), qb.data(), sizeof(int2) * (size_t)n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->pairQIv.get(), iv.data(), sizeof(int2) * iv.size(), hipMemcpyHostToDevice));
  HIPCHK(c, gtx::launch_pair_hit(c->pairQ.get(), c->pairQBlk.get(), c->pairQIv.get(), n, c->rx.pairAll.ix, ref_blocks(c), c->rx.pairAcc.get(),
                                 c->stream));
  c->pairUsed = true;
  return GTX_OK;
}

int gtxi_pairs_on(gtx_ctx *c) { return c && (c->rx.refBlocks || c->pairUsed) ? 1 : 0; }

// ---------------------------------------------------------------------------------------------
// coverage
// ---------------------------------------------------------------------------------------------
// bucket tables over ONE sorted array (the coverage thresholds): cuts every bucket_e_size() entries, never across classes; the slice
// a bucket keeps in LDS begins where the bucket does (a read ends at or behind its start) -- see the same for the two boundary
// arrays of the count path in gtx_set_refs_ex
static int cover_bucket_tables(gtx_ctx *c, const std::vector<int32_t> &sortedT, const std::vector<int32_t> &seg)
{
  const int nClasses = c->nClasses;
  const int kE = gtx::bucket_e_size(), kS = gtx::bucket_t_size();
  BucketCuts k;
  k.clsStart.assign(nClasses + 1, 0);
  for (int cl = 0; cl < nClasses; cl++) {
    k.clsStart[cl] = (int32_t)k.posHi.size();
    const int32_t s0 = seg[cl], s1 = seg[cl + 1];
    for (int32_t e0 = s0; e0 < s1; e0 += kE) {
      const int32_t e1 = (int32_t)std::min<int64_t>((int64_t)e0 + kE, s1);
      k.posHi.push_back(e1 == s1 ? INT32_MAX : sortedT[e1 - 1]);
      k.eLo.push_back(e0); k.eHi.push_back(e1); k.cls.push_back(cl);
      k.sLo.push_back(e0); k.sHi.push_back((int32_t)std::min<int64_t>((int64_t)e0 + kS, s1));
    }
  }
  k.clsStart[nClasses] = (int32_t)k.posHi.size();
  if (k.posHi.size() > 8192 || nClasses > 2048) { c->cv.bkt.nB = 0; return GTX_OK; }
  return build_bucket_tables(c, c->cv.bkt, k, nClasses);
}

static int cover_prepare(gtx_ctx *c)
{
  if (c->cv.ready) return GTX_OK;
  // the thresholds of every region that takes part (the rule of gtx_set_refs_ex): E_k and S_k - 1, sorted by (class, value)
  const int64_t m = c->nRefs;
  struct Item { int32_t cls, val, k2; };                      // k2 = 2 * region + (0: the E threshold, 1: the S - 1 threshold)
  std::vector<Item> it;
  it.reserve((size_t)2 * c->nValid);
  for (int64_t k = 0; k < m; k++) {
    const int32_t cl = c->h_refC[k], s = c->h_refS[k], e = c->h_refE[k];
    const bool take = cl >= 0 && (c->mergeRefs ? (int64_t)s <= (int64_t)e + 1 : !(s > e || e <= 0));
    if (!take) continue;
    it.push_back({cl, e, (int32_t)(2 * k)}); it.push_back({cl, s - 1, (int32_t)(2 * k + 1)});
  }
  std::sort(it.begin(), it.end(), [](const Item &a, const Item &b) { return a.cls != b.cls ? a.cls < b.cls : (a.val != b.val ? a.val < b.val : a.k2 < b.k2); });
  const int64_t nt = (int64_t)it.size();
  std::vector<int32_t> sortedT(nt + 1), seg(c->nClasses + 1, 0), posTE(m > 0 ? m : 1, -1), posTS(m > 0 ? m : 1, -1), base(m > 0 ? m : 1, -1);
  for (int64_t i = 0; i < nt; i++) seg[it[i].cls + 1]++;
  for (int cl = 0; cl < c->nClasses; cl++) seg[cl + 1] += seg[cl];
  for (int64_t i = 0; i < nt; i++) {
    sortedT[i] = it[i].val;
    const int32_t k = it[i].k2 >> 1;
    ((it[i].k2 & 1) ? posTS : posTE)[k] = (int32_t)(i + it[i].cls);          // histogram slot = rank + class id, as in gtx_set_refs_ex
    base[k] = seg[it[i].cls] + it[i].cls - 1;
  }
  const int64_t nTop = (nt + 255) >> 8;
  std::vector<int32_t> topT(nTop + 1);
  for (int64_t i = 0; i < nTop; i++) topT[i] = sortedT[i << 8];
  c->cv.histLenT = nt + c->nClasses;
  const int nTiles = gtx::scan_tiles(c->cv.histLenT);
  HIPCHK(c, c->cv.sortedT.alloc(nt + 1));
  HIPCHK(c, c->cv.segT.alloc(c->nClasses + 1));
  HIPCHK(c, c->cv.topT.alloc(nTop + 1));
  HIPCHK(c, c->cv.posTE.alloc(m + 1));
  HIPCHK(c, c->cv.posTS.alloc(m + 1));
  HIPCHK(c, c->cv.classBaseT.alloc(m + 1));
  HIPCHK(c, hipMemcpy(c->cv.sortedT.get(), sortedT.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->cv.segT.get(), seg.data(), sizeof(int32_t) * (c->nClasses + 1), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->cv.topT.get(), topT.data(), sizeof(int32_t) * (nTop + 1), hipMemcpyHostToDevice));
  if (m > 0) {
    HIPCHK(c, hipMemcpy(c->cv.posTE.get(), posTE.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->cv.posTS.get(), posTS.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->cv.classBaseT.get(), base.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
  }
  for (int q = 0; q < 4; q++) {
    HIPCHK(c, c->cv.cov[q].alloc(c->cv.histLenT));          // histograms
    HIPCHK(c, c->cv.cov[4 + q].alloc(nTiles + 2));         // tile sums
    HIPCHK(c, c->cv.cov[8 + q].alloc(c->cv.histLenT));      // prefixes
    HIPCHK(c, hipMemset(c->cv.cov[q].get(), 0, sizeof(u64) * c->cv.histLenT));
    HIPCHK(c, hipMemset(c->cv.cov[4 + q].get(), 0, sizeof(u64) * (nTiles + 2)));
  }
  { int rc = ref_columns(c); if (rc) return rc; }
  { int rc = cover_bucket_tables(c, sortedT, seg); if (rc) return rc; }
  { int rc = make_place_table(c, seg, sortedT, sortedT, c->nClasses, nt, c->cv.place); if (rc) return rc; }
  c->cv.ready = true; c->covDirty = false;
  return GTX_OK;
}

static gtx::CoverArgs cover_args(gtx_ctx *c, int64_t nReads, int64_t indexBase = 0, uint32_t flags = 0)
{
  gtx::CoverArgs a;
  a.indexBase = indexBase;
  a.sortedT = c->cv.sortedT.get(); a.segStartT = c->cv.segT.get(); a.topT = c->cv.topT.get();
  for (int q = 0; q < 4; q++) { a.hist[q] = c->cv.cov[q].get(); a.part[q] = c->cv.cov[4 + q].get(); }
  a.info = c->d_info.get() + c->infoCur; a.nClasses = c->nClasses;
  const bool merge = (flags & GTX_ZERO_LENGTH_OK) && (flags & GTX_GAPS_FORMULA) && c->mergeRefs && c->side.get();
  a.side = merge ? c->side.get() : nullptr; a.sideCount = merge ? c->sideCount.get() : nullptr; a.sideCap = c->sideCap;
  a.wfast = gtx::route_knobs().weightedFast ? 1 : 0;
  a.chunksPerWave = gtx::cover_chunks_per_wave(nReads, c->chunksPerWave);
  a.sched = gtx::span_schedule((nReads + 63) >> 6, a.chunksPerWave, 4, c->waveSlots);
  a.place = c->cv.place.view();
  return a;
}

static int cover_begin(gtx_ctx *c)
{
  int rc = cover_prepare(c); if (rc) return rc;
  if (c->covDirty) {
    const int nTiles = gtx::scan_tiles(c->cv.histLenT);
    for (int q = 0; q < 4; q++) {
      HIPCHK(c, hipMemsetAsync(c->cv.cov[q].get(), 0, sizeof(u64) * c->cv.histLenT, c->stream));
      HIPCHK(c, hipMemsetAsync(c->cv.cov[4 + q].get(), 0, sizeof(u64) * (nTiles + 2), c->stream));
    }
  }
  if (c->covDirty || c->histDirty) {
    HIPCHK(c, hipMemcpyAsync(c->d_info.get() + c->infoCur, &c->h_info.get()[1], sizeof(gtx::DevInfo), hipMemcpyHostToDevice, c->stream));
    if (c->sideCount.get()) {
      HIPCHK(c, hipMemsetAsync(c->sideCount.get(), 0, sizeof(unsigned), c->stream));
      if (c->rx.nSpecial) HIPCHK(c, hipMemsetAsync(c->rx.specialOut.get(), 0, sizeof(u64) * c->rx.nSpecial, c->stream));
    }
  }
  c->sideUsed = false;
  c->covDirty = true; c->covTileSums = true;
  return GTX_OK;
}

} // extern "C"

// One batch of reads into the four coverage histograms: the streaming kernel (exact for any order, fast for sorted reads), or --
// for a batch the caller (GTX_READS_UNSORTED) or a sample of the host buffer says is in no particular order -- the partition path.
int cover_launch(gtx_ctx *c, const void *dR, const int *dW, int64_t n, int64_t indexBase, uint32_t flags, bool unsorted)
{
  const gtx::CoverArgs cv = cover_args(c, n, indexBase, flags);
  gtx::BucketPlan p; gtx::BucketWork w; bool part = false;
  if (unsorted) { int rc = partition_plan(c, c->cv.bkt, n, c->nClasses, dW != nullptr, &p, &w, &part); if (rc) return rc; }
  if (part) {
    gtx::CountArgs a = {};                                        // what the partition pass reads of it
    a.nClasses = c->nClasses; a.zeroLenOk = 0; a.coverRule = 1; a.info = cv.info; a.indexBase = indexBase;
    a.side = cv.side; a.sideCount = cv.sideCount; a.sideCap = cv.sideCap;
    HIPCHK(c, gtx::launch_cover_bucketed(dR, dW, n, a, cv, c->cv.bkt.view(), w, p, c->stream));
    c->covTileSums = false;
    return GTX_OK;
  }
  HIPCHK(c, gtx::launch_coverage(dR, dW, n, cv, c->stream));
  return GTX_OK;
}

// a host buffer's order, from 4096 adjacent pairs: a few descents are a few sorted runs (still the streaming kernel's business)
bool host_reads_look_unsorted(const int32_t *tri, int64_t n)
{
  if (n < 2) return false;
  const int64_t stride = n > 4096 ? n / 4096 : 1;
  int descents = 0;
  for (int64_t i = 0; i + 1 < n; i += stride) {
    const int32_t *a = tri + 3 * i, *b = a + 3;
    if ((b[0] < a[0] || (b[0] == a[0] && b[1] < a[1])) && ++descents > 8) return true;
  }
  return false;
}

extern "C" {

static int cover_end(gtx_ctx *c, void *d_cov_out)
{
  gtx::CoverGather g;
  for (int q = 0; q < 4; q++) { g.pref[q] = c->cv.cov[8 + q].get(); g.part[q] = c->cv.cov[4 + q].get(); }
  g.posTE = c->cv.posTE.get(); g.posTS = c->cv.posTS.get(); g.classBaseT = c->cv.classBaseT.get(); g.refS = c->rx.refS.get(); g.refE = c->rx.refE.get();
  if (!c->covTileSums)                                               // (the partition path does not keep them)
    for (int q = 0; q < 4; q += 2) HIPCHK(c, gtx::launch_tile_sums(c->cv.cov[q].get(), c->cv.cov[q + 1].get(), c->cv.histLenT, c->cv.cov[4 + q].get(), c->cv.cov[5 + q].get(), c->stream));
  HIPCHK(c, gtx::launch_coverage_finalize(cover_args(c, 0), c->cv.histLenT, g, c->nRefs, (u64 *)d_cov_out, c->d_info.get() + (c->infoCur ^ 1), c->stream));
  { int rc = merge_end(c, d_cov_out); if (rc) return rc; }
  c->covDirty = false;
  c->infoCur ^= 1;
  return GTX_OK;
}

int gtx_coverage_device(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, uint32_t flags, void *d_cov)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_coverage_device: gtx_set_refs has not been called");
  if (n < 0 || (n > 0 && !d_reads) || (c->nRefs > 0 && !d_cov)) return fail(c, GTX_E_ARG, "gtx_coverage_device: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = cover_begin(c); if (rc) return rc;
  prof_begin(c);
  HIPCHK(c, prof_mark(c, 1, c->stream));
  if (flags & GTX_GAPS_FORMULA) { rc = merge_prepare(c, flags, 2); if (rc) return rc; }
  rc = cover_launch(c, d_reads, (const int *)d_weights, n, 0, flags, (flags & GTX_READS_UNSORTED) != 0); if (rc) return rc;
  rc = merge_batch(c, d_reads, d_weights, n); if (rc) return rc;
  HIPCHK(c, prof_mark(c, 2, c->stream));
  rc = cover_end(c, d_cov); if (rc) return rc;
  HIPCHK(c, prof_end(c, c->stream));
  return GTX_OK;
}

int gtx_coverage_begin(gtx_ctx *c)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_coverage_begin: gtx_set_refs has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = cover_begin(c); if (rc) return rc;
  c->streamSeen = 0; c->covOpen = true;
  return GTX_OK;
}

int gtx_coverage_add(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, uint32_t flags)
{
  if (!c) return GTX_E_ARG;
  if (!c->covOpen) return fail(c, GTX_E_STATE, "gtx_coverage_add: gtx_coverage_begin has not been called");
  if (n < 0 || (n > 0 && !reads)) return fail(c, GTX_E_ARG, "gtx_coverage_add: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t seen = c->streamSeen;
  int rc = GTX_OK;
  if (flags & GTX_GAPS_FORMULA) { rc = merge_prepare(c, flags, 2); if (rc) return rc; }
  rc = stage_batches(c, reads, weights, n, [&](const void *dR, const int *dW, int64_t cnt, int64_t off) -> int {
    const bool unsorted = (flags & GTX_READS_UNSORTED) || (!(flags & GTX_READS_SORTED) && host_reads_look_unsorted(reads + 3 * off, cnt));
    { int rc2 = cover_launch(c, dR, dW, cnt, seen + off, flags, unsorted); if (rc2) return rc2; }
    return merge_batch(c, dR, dW, cnt);
  });
  if (rc) return rc;
  c->streamSeen += n;
  return GTX_OK;
}

int gtxi_coverage_finish(gtx_ctx *c, void **d_out)
{
  if (!c->covOpen) return fail(c, GTX_E_STATE, "gtx_coverage_end: gtx_coverage_begin has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  c->covOpen = false; c->seamUnsorted = INT64_MAX;
  int rc = ensure_out(c, (size_t)c->nRefs); if (rc) return rc;
  rc = cover_end(c, c->out.get()); if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(&c->h_info.get()[0], c->d_info.get() + (c->infoCur ^ 1), sizeof(gtx::DevInfo), hipMemcpyDeviceToHost, c->stream));
  *d_out = c->out.get();
  return GTX_OK;
}

int gtx_coverage_end(gtx_ctx *c, uint64_t *cov, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->covOpen && c->nRefs > 0 && !cov) return fail(c, GTX_E_ARG, "gtx_coverage_end: null output");
  void *d = nullptr;
  int rc = gtxi_coverage_finish(c, &d); if (rc) return rc;
  if (c->nRefs > 0) HIPCHK(c, hipMemcpyAsync(cov, d, sizeof(u64) * c->nRefs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
  if (info) gtxi_fetch_info(c, info);
  return GTX_OK;
}

int gtx_coverage(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, uint32_t flags, uint64_t *cov, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (n < 0 || (n > 0 && !reads)) return fail(c, GTX_E_ARG, "gtx_coverage: bad argument");
  int rc = gtx_coverage_begin(c); if (rc) return rc;
  rc = gtx_coverage_add(c, reads, weights, n, flags); if (rc) { c->covOpen = false; return rc; }
  return gtx_coverage_end(c, cov, info);
}

// A group member's share: the classes `owned` (flags per class).  tiles = the 1024-slot histogram tiles that hold a slot of an
// owned class or the slot just below its first (class c has slots seg[c]+c-1 .. seg[c+1]+c: the gather reads the prefix at the
// slot below as the class's base); regions = `regions[0..nRegions)`, the file indices of the member's regions in the group's
// compact order, its piece beginning at compact position `offset`.
int gtxi_set_share(gtx_ctx *c, const uint8_t *owned, int32_t nClasses, const int32_t *regions, int64_t nRegions, int64_t offset)
{
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtxi_set_share: gtx_set_refs has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int nTilesAll = gtx::scan_tiles(c->histLen);
  std::vector<uint8_t> mark(nTilesAll > 0 ? nTilesAll : 1, 0);
  for (int cl = 0; cl < c->nClasses && cl < nClasses; cl++) {
    if (!owned[cl] || c->h_seg[cl] == c->h_seg[cl + 1]) continue;
    const int64_t lo = std::max<int64_t>(0, (int64_t)c->h_seg[cl] + cl - 1), hi = (int64_t)c->h_seg[cl + 1] + cl;   // slots lo..hi
    for (int64_t t = lo >> 10; t <= (hi >> 10) && t < nTilesAll; t++) mark[t] = 1;
  }
  std::vector<int32_t> tiles;
  for (int t = 0; t < nTilesAll; t++) if (mark[t]) tiles.push_back(t);
  c->share.tiles.reset(); c->share.regions.reset(); c->share.owned.reset();
  {
    std::vector<uint8_t> own((size_t)std::max(c->nClasses, 1), 0);
    for (int cl = 0; cl < c->nClasses && cl < nClasses; cl++) own[cl] = owned[cl] ? 1 : 0;
    HIPCHK(c, c->share.owned.alloc(own.size()));
    HIPCHK(c, hipMemcpy(c->share.owned.get(), own.data(), own.size(), hipMemcpyHostToDevice));
  }
  HIPCHK(c, c->share.tiles.alloc(tiles.size() + 1));
  HIPCHK(c, c->share.regions.alloc((size_t)(nRegions + 1)));
  if (!tiles.empty()) HIPCHK(c, hipMemcpy(c->share.tiles.get(), tiles.data(), sizeof(int32_t) * tiles.size(), hipMemcpyHostToDevice));
  if (nRegions > 0) HIPCHK(c, hipMemcpy(c->share.regions.get(), regions, sizeof(int32_t) * (size_t)nRegions, hipMemcpyHostToDevice));
  c->share.nTiles = (int)tiles.size(); c->share.nRegions = nRegions; c->share.offset = offset; c->share.on = true;
  return ensure_out(c, GTXI_SHARE_SLOTS * (size_t)c->nRefs);     // the compact vectors gtxi_count_device_share[_async] takes in turn (slot)
}

// gtx_count_device for a group member: the reads (of the member's classes, resident on its device) are counted and the member's
// regions finalized into its piece of compact vector `slot` (0 | 1), c->out.get() + slot * nRefs + shareOffset.  Enqueued on the
// context's stream.
int gtxi_count_device_share(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, uint32_t flags, int slot, void *direct_out, void **d_piece, int64_t *pieceLen)
{
  if (!c->share.on) return fail(c, GTX_E_STATE, "gtxi_count_device_share: no share set");
  if (c->rx.refBlocks) return fail(c, GTX_E_STATE, "gtx_group_count_device: multi-interval regions (gtx_set_ref_blocks) are outside the members' shares");
  if (n < 0 || (n > 0 && !d_reads)) return fail(c, GTX_E_ARG, "gtx_group_count_device: bad argument");
  if (flags & GTX_ZERO_LENGTH_OK) return fail(c, GTX_E_ARG, "gtx_group_count_device: GTX_ZERO_LENGTH_OK (sorted-merge semantics with their host-side corrections) is served by the host-buffer group calls only");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = count_begin(c); if (rc) return rc;
  prof_begin(c);
  HIPCHK(c, prof_mark(c, 1, c->stream));
  const bool streaming = (flags & (GTX_READS_SORTED | GTX_CHECK_SORTED)) != 0;
  if (!streaming) c->tileSumsValid = false;
  if (n > 0) {
    if (streaming) HIPCHK(c, gtx::launch_count(d_reads, d_weights, n, count_args(c, c->ix.hist, flags, n, 0, COUNT_SHARE), true, c->stream));
    else { rc = launch_unsorted(c, d_reads, d_weights, n, count_args(c, c->ix.hist, flags, n, 0, COUNT_SHARE)); if (rc) return rc; }
  }
  HIPCHK(c, prof_mark(c, 2, c->stream));
  u64 *dst = direct_out ? (u64 *)direct_out : c->out.get() + (size_t)(slot % GTXI_SHARE_SLOTS) * c->nRefs + c->share.offset;
  rc = count_end(c, dst, true, direct_out != nullptr); if (rc) return rc;
  HIPCHK(c, prof_end(c, c->stream));
  *d_piece = dst; *pieceLen = c->share.nRegions;
  return GTX_OK;
}

// The same for reads in stream order, without a wait between successive calls: the streaming kernel and the finalize step of the
// member's share run on `run` -- the group alternates between two streams of its own, so that the kernel of call k+1 is not ordered
// behind the kernel of call k and takes the wave slots its tail frees -- with histogram set `set` (0 | 1: one per stream; the stream's
// order is what keeps call k+2's kernel out of what call k's finalize step is scanning and zeroing).  The finalize step writes the
// member's piece of compact vector `slot`; the caller has made `run` wait for whatever last read that piece.
static constexpr int kInfoRing = 2 * GTXI_SHARE_STREAMS;
int gtxi_count_device_share_async(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, uint32_t flags, int slot, int set, hipStream_t run,
                                  void *direct_out, void **d_piece, int64_t *pieceLen)
{
  if (!c->share.on) return fail(c, GTX_E_STATE, "gtxi_count_device_share_async: no share set");
  if (c->rx.refBlocks || (flags & GTX_ZERO_LENGTH_OK) || !(flags & GTX_READS_SORTED) || n < 0 || (n > 0 && !d_reads))
    return fail(c, GTX_E_ARG, "gtxi_count_device_share_async: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  HistSet &h = c->ix.alt[set % GTXI_SHARE_STREAMS];
  if (!h.flags) { int rc = make_hist_set(c, h, c->histLen); if (rc) return rc; }
  if (!c->ix.info3) {
    HIPCHK(c, c->ix.info3.alloc(kInfoRing));
    for (int k = 0; k < kInfoRing; k++) HIPCHK(c, hipMemcpy(c->ix.info3.get() + k, &c->h_info.get()[1], sizeof(gtx::DevInfo), hipMemcpyHostToDevice));
  }
  // info blocks: the calls on stream `set` take two blocks in turn; a call's finalize step clears the other one -- the block of the
  // call that ran on this stream before, for the call that runs on it next
  const int st = set % GTXI_SHARE_STREAMS;
  const unsigned turn = c->ix.shareTurn[st]++;
  c->ix.shareSeq++;
  gtx::DevInfo *info = c->ix.info3.get() + 2 * st + (turn & 1), *infoNext = c->ix.info3.get() + 2 * st + ((turn + 1) & 1);
  prof_begin(c);
  HIPCHK(c, prof_mark(c, 1, run));
  const bool keepDefault = c->tileSumsValid;
  c->tileSumsValid = true;
  gtx::CountArgs a = count_args(c, h, flags, n, 0, COUNT_SHARE_ASYNC, d_weights == nullptr);   // (clears c->tileSumsValid when the kernel leaves the tile sums to the finalize step)
  a.info = info;
  const bool sumsValid = c->tileSumsValid;
  c->tileSumsValid = keepDefault;
  if (n > 0) HIPCHK(c, gtx::launch_count(d_reads, d_weights, n, a, true, run));
  HIPCHK(c, prof_mark(c, 2, run));
  // direct_out (may be null): the caller's result vector in file order (n_refs entries) -- the member's regions go to their places in it
  u64 *dst = direct_out ? (u64 *)direct_out : c->out.get() + (size_t)(slot % GTXI_SHARE_SLOTS) * c->nRefs + c->share.offset;
  const gtx::FinalizeShare fs = {c->share.tiles.get(), c->share.nTiles, c->share.regions.get(), c->share.nRegions, direct_out != nullptr};
  int rc = finalize_set(c, h, sumsValid, dst, info, infoNext, run, &fs, a.hist32 != 0 && n > 0); if (rc) return rc;
  HIPCHK(c, prof_end(c, run));
  c->ix.lastShareInfo = info;
  *d_piece = dst; *pieceLen = c->share.nRegions;
  return GTX_OK;
}

// For the tests of the two-launch finalize: how many words of the tile totals that the NEXT such finalize on a set will write are not
// zero (the invariant between calls: none -- the gather of the call before zeroed them).  set < 0: the context's own set, else the
// group's set `set`.  Waits for the device.
int gtxi_next_totals_nonzero(gtx_ctx *c, int set, int64_t *nonzero)
{
  if (!c || !nonzero) return GTX_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  const HistSet &h = set < 0 ? c->ix.hist : c->ix.alt[set % GTXI_SHARE_STREAMS];
  *nonzero = 0;
  if (!h.totals) return GTX_OK;
  const size_t pair = h.totals.cap / 2;                              // one turn's totals: both histograms
  std::vector<u64> host(pair);
  HIPCHK(c, hipMemcpy(host.data(), h.totals.get() + (size_t)(h.totalsTurn & 1) * pair, sizeof(u64) * pair, hipMemcpyDeviceToHost));
  for (u64 v : host) *nonzero += v != 0;
  return GTX_OK;
}

// what the last gtxi_count_device_share_async call observed (the caller has waited for its streams)
int gtxi_last_share_info(gtx_ctx *c, gtx_count_info *info)
{
  if (!c->ix.lastShareInfo) return gtx_last_info(c, info);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy(&c->h_info.get()[0], c->ix.lastShareInfo, sizeof(gtx::DevInfo), hipMemcpyDeviceToHost));
  info_out(c->h_info.get()[0], info, 0);
  return fault_check(c, c->h_info.get()[0]);
}

void *gtxi_out_buffer(gtx_ctx *c) { return c->out.get(); }
int gtxi_ensure_out(gtx_ctx *c, int64_t n)
{
  HIPCHK(c, hipSetDevice(c->device));
  if ((size_t)n > c->out.cap) HIPCHK(c, hipStreamSynchronize(c->stream));      // (the old vector may still be read)
  return ensure_out(c, (size_t)std::max<int64_t>(n, 0));
}
// a second device buffer of the context (grown, never shrunk): where a group's member 0 assembles a result
int gtxi_scratch(gtx_ctx *c, size_t bytes, void **p)
{
  HIPCHK(c, hipSetDevice(c->device));
  if (bytes > c->scratch.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->scratch.reserve(bytes));
  }
  *p = c->scratch.get();
  return GTX_OK;
}

// a DMA out of the caller's page-locked buffer may still be in flight (stage_batches returns with it enqueued): wait for it
int gtxi_wait_direct(gtx_ctx *c)
{
  if (c->stage.directPending) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->stage.copyStream)); c->stage.directPending = false; }
  return GTX_OK;
}

hipStream_t gtxi_stream(gtx_ctx *c) { return c->stream; }
int gtxi_device(gtx_ctx *c) { return c->device; }
void gtxi_set_error(gtx_ctx *c, const char *msg) { c->err = msg; }

// ---------------------------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------------------------
int gtx_profile_enable(gtx_ctx *c, int on)
{
  if (!c || on < 0) return GTX_E_ARG;
  c->prof.on = on != 0; c->prof.every = on > 1 ? on : 1; c->prof.calls = 0; c->prof.seq = 0; c->prof.profThis = false;
  return GTX_OK;
}

int gtx_profile_read(gtx_ctx *c, int back, float *msKernel, float *msTotal)
{
  if (!c) return GTX_E_ARG;
  if (back < 0 || back >= Profile::kSlots || back >= c->prof.calls) return fail(c, GTX_E_STATE, "gtx_profile_read: no such profiled call");
  HIPCHK(c, hipSetDevice(c->device));
  hipEvent_t *ev = c->prof.ring[(c->prof.calls - 1 - back) % Profile::kSlots];
  const bool kernelOnly = c->prof.every > 1;
  HIPCHK(c, hipEventSynchronize(ev[kernelOnly ? 2 : 3]));
  float a = 0, b = 0;
  HIPCHK(c, hipEventElapsedTime(&a, ev[1], ev[2]));
  if (kernelOnly) b = a; else HIPCHK(c, hipEventElapsedTime(&b, ev[1], ev[3]));
  if (msKernel) *msKernel = a;
  if (msTotal) *msTotal = b;
  return GTX_OK;
}

int gtx_profile_last(gtx_ctx *c, float *msKernel, float *msTotal) { return gtx_profile_read(c, 0, msKernel, msTotal); }

int gtx_profile_count(gtx_ctx *c) { return c ? (int)std::min<long long>(c->prof.calls, Profile::kSlots) : 0; }

} // extern "C"
