// gtx_capi.hip -- implementation of the C ABI declared in include/gtx.h.
//
// Host side of the engine: builds the device-resident rank structure from the reference
// regions (replacing the bin-index construction of UnsortedGenomicRegionSetOverlaps,
// gtools/genomic_intervals.cpp:5593-5675), enqueues the streaming count / scan kernels of
// gtx_kernels.hip, and moves buffers.  There is deliberately no CPU implementation of the
// counting path in this library: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "gtx.h"
#include "gtx_kernels.h"
#include "gtx_pairs.h"
#include "gtx_join.h"
#include "gtx_query.h"
#include "gtx_offset.h"
#include "gtx_annotate.h"
#include "gtx_signal.h"
#include "gtx_text.h"
#include "gtx_link.h"
#include "gtx_adjacent.h"
#include "gtx_select.h"
#include "gtx_internal.h"

typedef unsigned long long u64;

static thread_local std::string g_create_error;

namespace {

// A buffer of T in device memory (Pinned: in page-locked host memory) that frees itself; move-only.  cap = elements it holds.
template <class T, bool Pinned> class Buf {
 public:
  size_t cap = 0;
  Buf() = default;
  Buf(Buf &&o) noexcept { *this = std::move(o); }
  Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); std::swap(cap, o.cap); std::swap(p_, o.p_); } return *this; }
  ~Buf() { reset(); }
  T *get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; cap = 0; }
  // exactly n elements (the one-shot tables); what it held is freed first
  hipError_t alloc(size_t n)
  {
    reset();
    const hipError_t e = Pinned ? hipHostMalloc((void **)&p_, sizeof(T) * n) : hipMalloc((void **)&p_, sizeof(T) * n);
    if (e == hipSuccess) cap = n;
    return e;
  }
  // grown, never shrunk: when `need` elements are more than it holds, free, then allocate `room` (>= need) and count `need` as held
  hipError_t reserve(size_t need, size_t room) { if (need <= cap) return hipSuccess; hipError_t e = alloc(room); if (e == hipSuccess) cap = need; return e; }
  hipError_t reserve(size_t n) { return reserve(n, n); }
  hipError_t grow(size_t n) { return reserve(std::max<size_t>(n, 1)); }   // ... and never empty
 private:
  T *p_ = nullptr;
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinBuf = Buf<T, true>;

// direct placement at the start of a span (gtx::PlaceTable): per class {segment start, end, first cell, cells}; per cell the rank
// of the cell's first position in the ends array and in the starts array
struct PlaceTable {
  DevBuf<int4> cls; DevBuf<int> rank; int shift = 0;
  gtx::PlaceTable view() const { gtx::PlaceTable t; t.cls = cls.get(); t.rank = rank.get(); t.shift = shift; return t; }
};

// the direct-address bucket lookup of the partition path (gtx::BucketTable): posHi | eLo | eHi | sLo | sHi | cls (nB each) |
// clsStart (nClasses+1) in `bkt`, the cells of each class, the first bucket of each cell.  nB = 0: no tables (the search kernel serves)
struct BucketTables {
  DevBuf<int> bkt; DevBuf<int4> clsCell; DevBuf<uint16_t> cellTab; int nB = 0, nCells = 0, cellShift = 0;
  gtx::BucketTable view() const
  {
    gtx::BucketTable t;
    const int *d = bkt.get();
    t.posHi = d; t.eLo = d + nB; t.eHi = d + 2 * nB; t.sLo = d + 3 * nB; t.sHi = d + 4 * nB; t.cls = d + 5 * nB; t.clsStart = d + 6 * nB; t.nB = nB;
    t.clsCell = clsCell.get(); t.cellTab = cellTab.get(); t.nCells = nCells; t.cellShift = cellShift;
    return t;
  }
};

// the cuts of a partition path's buckets: per bucket the largest read start it takes, its ranges of the two boundary arrays, its
// class; per class its first bucket
struct BucketCuts { std::vector<int32_t> posHi, eLo, eHi, sLo, sHi, cls, clsStart; };

// histograms, tile sums, prefix arrays of one count call and the finalize_scan_chained_kernel's flags (one per tile and histogram)
// with the call's epoch; the tiles' totals of the two-launch finalize (finalize_local_kernel), two per histogram, and whose turn it is
struct HistSet {
  DevBuf<u64> histA, histB, partA, partB, prefA, prefB; DevBuf<unsigned> flags; unsigned epoch = 0; unsigned long long draws = 0;
  DevBuf<u64> totals; unsigned totalsTurn = 0;
  gtx::FinalizeArgs view(int64_t histLen) const
  {
    gtx::FinalizeArgs a = {};
    const size_t turn = 2 * ((size_t)gtx::scan_tiles(histLen) + 2);      // words of one turn's totals
    a.histA = histA.get(); a.histB = histB.get(); a.tileA = partA.get(); a.tileB = partB.get(); a.prefA = prefA.get(); a.prefB = prefB.get(); a.histLen = histLen;
    a.chainFlags = flags.get(); a.epoch = epoch; a.draws = draws;
    a.totals = totals.get() + (totalsTurn & 1) * turn; a.nextTotals = totals.get() + ((totalsTurn & 1) ^ 1) * turn;
    return a;
  }
};

// What a reference set is made into, in four parts that gtx_set_refs_ex drops together (by assignment) before it makes them anew.
// The count index: sorted boundary arrays, the search kernel's top levels, placement, the partition path's tables, the histograms
struct CountIndex {
  DevBuf<int> sortedE, sortedS, segStart, posE, posS, classBase;
  DevBuf<int> sampE, sampS; int sampShift = 6, nSamp = 0;   // top level of the search kernel
  DevBuf<int> topE, topS;                          // every 256th boundary: first hop of the streaming kernel's start-of-span search
  PlaceTable place;
  BucketTables bkt;                                // unsorted reads, partition path (gtx_bucket.hip)
  HistSet hist;
  // The group's device calls (gtxi_count_device_share_async) finalize call k on the group's exchange stream UNDER the streaming kernel
  // of call k+1: more sets of histograms, tile sums, prefix arrays and chain flags in turn (never `hist`: the other entry points
  // stay as they are), two info blocks per stream (a call's finalize step resets the other one)
  HistSet alt[GTXI_SHARE_STREAMS];                 // (dropped with the set: the ring of info blocks restarts clean)
  DevBuf<gtx::DevInfo> info3; unsigned shareSeq = 0; unsigned shareTurn[GTXI_SHARE_STREAMS] = {}; const gtx::DevInfo *lastShareInfo = nullptr;
};

// coverage (made on first use, cover_prepare): the merged threshold array of the regions (E_k and S_k - 1, sorted per class) with its
// 4 histograms, 4 tile-sum arrays, 4 prefix arrays, and its own placement and partition tables
struct CoverIndex {
  DevBuf<u64> cov[12];
  DevBuf<int> sortedT, segT, topT, posTE, posTS, classBaseT;
  int64_t histLenT = 0;
  PlaceTable place;
  BucketTables bkt;
  bool ready = false;
};

// the rest that hangs on the reference set: region coordinates in file order, the inverted regions, multi-interval regions, the
// join's order keys, pair offsets' reference points and strands, signal bins' lengths
struct RefExtras {
  DevBuf<int> refS, refE, refC;
  // sorted-merge semantics, intervals with start > end + 1 (gtx_special.hip): the K inverted reference regions and their sums
  int nSpecial = 0; DevBuf<int4> specialRefs; DevBuf<int> specialIdx; DevBuf<u64> specialOut;
  // count without -gaps over multi-interval regions (gtx_pairs.hip): envelope indexes over the multi-interval index regions
  // (reads with one interval are checked against them batch by batch) and over all regions (made on the first multi-interval
  // read), the regions' interval lists, and the two correction vectors add[nRefs] | sub[nRefs] (zero between calls)
  struct PairIdx { DevBuf<int> mem; int n = 0; bool built = false; gtx::PairIndex ix = {}; } pairMulti, pairAll;
  DevBuf<int2> blkOf, blkIv; bool refBlocks = false;
  DevBuf<u64> pairAcc;
  // the overlap join (gtx_join.hip) over the envelope index pairAll: the regions' order keys (host copy too), whether the index
  // is already in key order (-1: not yet looked at)
  DevBuf<long long> joinKey; std::vector<long long> h_joinKey; int joinMono = -1;
  DevBuf<int4> offRef; DevBuf<int8_t> refStrand;   // pair offsets: per-ordinal front / back interval, strands (gtx_set_ref_strands)
  // signal bins (gtx_signal.hip): the geometry of gtx_set_signal_bins, per-ordinal reference lengths
  bool sigSet = false; double sigMin = 0, sigMax = 0; int64_t sigBins = 0; DevBuf<long long> sigRefLen;
};

// a group member's share of the finalize step (gtxi_set_share): tiles of its classes, its regions in the group's compact order
struct Share { bool on = false; DevBuf<int> tiles; int nTiles = 0; DevBuf<int> regions; int64_t nRegions = 0, offset = 0; DevBuf<unsigned char> owned; };

// a block of region text tokenised on the device (gtx_count_add_text)
struct TextSlot {
  DevBuf<char> text; DevBuf<unsigned> seg;
  DevBuf<unsigned> nl; DevBuf<int> tri, w;                    // w (made last) holds the lines these are made for
  DevBuf<int> tri2; DevBuf<unsigned> blk; DevBuf<int> w2;      // ... w2 those of the strand-aware outputs
  DevBuf<int> flag; PinBuf<int> hostFlag; PinBuf<char> pin, seam; DevBuf<unsigned long long> sum;
  hipEvent_t evParsed = nullptr, evConsumed = nullptr, evCopied = nullptr; bool busy = false;
  // gtx_subset_text: the lines' hits, the tiles' kept bytes / lines, the kept text and its
  // totals on the host; whether the slot holds a subset block whose result has not been fetched
  DevBuf<unsigned> hits; DevBuf<unsigned long long> tile; DevBuf<char> out; PinBuf<unsigned long long> hostTotal; bool subsetPending = false;
};

} // namespace

struct gtx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // reference side
  int64_t nRefs = -1, nValid = 0;
  int nClasses = 0;
  std::vector<int32_t> h_seg;                        // [nClasses+1] class segments of the sorted boundary arrays (host copy)
  CountIndex ix;                                     // made from the reference set (gtx_set_refs_ex)
  CoverIndex cv;
  RefExtras rx;
  Share share;
  bool covTileSums = true;                           // false: a batch went through the partition path, the tile sums are rebuilt before the finalize step
  DevBuf<u64> bktReads; DevBuf<int> bktWeights; DevBuf<unsigned> bktDir, bktCnt;   // scratch of the partition path (gtx::BucketWork)
  int64_t bucketMinReads = gtx::kBucketMinReads;    // below this the per-read search kernel is used (GTX_BUCKET_MIN_READS)
  int localMaxTiles = gtx::kLocalScanMaxTiles;       // tile sums not kept: local scan + gather up to this many tiles (GTX_LOCAL_SCAN_MAX_TILES; 0: tile sums + scan + gather)
  bool histDirty = false;              // a call was abandoned between begin and end
  bool covDirty = false, covOpen = false;
  std::vector<int32_t> h_refS, h_refE, h_refC;
  // the inverted reads the kernels set aside (sorted-merge semantics)
  bool mergeRefs = false;               // the reference set was given with GTX_REFS_KEEP_ZERO_LENGTH
  DevBuf<int4> side; DevBuf<unsigned> sideCount; int sideCap = 1 << 20; bool sideUsed = false;
  int specialMode = 0;                  // value of a pair in the open call: 0 count, 2 the -gaps coverage formula
  bool tileSumsValid = true;           // every kernel since the last finalize maintained the tile sums
  int64_t histLen = 0;
  bool pairUsed = false;
  DevBuf<int4> pairQ; DevBuf<int2> pairQBlk, pairQIv;
  // the overlap join's offsets / scan / pair buffers of the host-buffer entry, its queries
  DevBuf<long long> joinOff, joinPart, joinCut; DevBuf<int> joinPairs, joinScratch; DevBuf<unsigned> joinBig;
  DevBuf<int> joinReads; DevBuf<int2> joinQBlk, joinQIv;
  DevBuf<gtx::JoinInfo> joinInfo;
  DevBuf<unsigned> hitsOut;             // gtx_query_hits: a batch's hits
  int64_t joinBuffer = 1ll << 26;       // pairs per device chunk of gtx_join (gtx_set_join_buffer)
  DevBuf<long long> offInv, offOut, offCnt, offPart; DevBuf<int8_t> offQStrand;   // the pair offsets' host entry
  DevBuf<long long> annCnt, annVal; DevBuf<int> annRef;   // the annotate pass' host entry: a chunk's kept offsets, values and ordinals
  DevBuf<gtx::SignalInfo> sigInfo; DevBuf<unsigned long long> sigBins; DevBuf<long long> sigW;   // the signal bins' info block, the host entry's bins and weights

  // link: the scans' per-tile values and break bit map, the info block and its page-locked copy (handed to the caller's struct by
  // gtx_sync after a device call), the host entry's inputs and group records
  DevBuf<int2> linkAgg, linkPrefix; DevBuf<u64> linkBits; DevBuf<unsigned> linkHeads; DevBuf<long long> linkBase;
  DevBuf<gtx::LinkInfo> linkInfo; PinBuf<gtx::LinkInfo> linkHost; gtx_link_info *linkPending = nullptr;
  DevBuf<int> linkTri, linkStop; DevBuf<long long> linkVals, linkVal; DevBuf<unsigned> linkHead, linkCnt;
  // gtx_link_text_begin .. _end: the input collected on the device block by block, the strands beside it, the heads' keys
  bool linkTextOpen = false; int64_t linkTextN = 0, linkTextCap = 0; int linkTextChrom = 0, linkTextByStrand = 0;
  DevBuf<int> linkTextTri; DevBuf<unsigned char> linkMinus; DevBuf<int2> linkHeadKey;
  // the neighbour passes (gtx_adjacent / gtx_gaps): per-tile sums, per-span gap counts and bases, the class bounds, the info blocks
  // and their page-locked copies (handed over like link's), the host entries' inputs and outputs
  DevBuf<uint2> adjSums; DevBuf<unsigned> gapCount; DevBuf<long long> gapBase, gapBounds;
  DevBuf<gtx::AdjInfo> adjInfo; PinBuf<gtx::AdjInfo> adjHost; gtx_adjacent_info *adjPending = nullptr;
  DevBuf<gtx::GapInfo> gapInfo; PinBuf<gtx::GapInfo> gapHost; gtx_gaps_info *gapPending = nullptr;
  DevBuf<int> adjTri, gapStart, gapStop; DevBuf<unsigned char> adjMinus; DevBuf<long long> adjDist; DevBuf<unsigned> gapOwner;

  DevBuf<gtx::DevInfo> d_info;          // 2 blocks: the finalize of one call resets the block of the next
  int infoCur = 0;
  PinBuf<gtx::DevInfo> h_info;          // [0] = readback, [1] = init pattern

  // staging for the host-buffer entry points: two device slots fed from two pinned host slots by a copy stream, so that
  // the host->device copy of batch i+1 runs under the kernels of batch i (Stage* functions below)
  hipStream_t copyStream = nullptr;
  DevBuf<char> stage[2]; DevBuf<int> stageW[2];   // (12 bytes per read)
  PinBuf<char> pin[2];                            // bytes per slot
  hipEvent_t evCopied[2] = {nullptr, nullptr}, evConsumed[2] = {nullptr, nullptr}; bool slotBusy[2] = {false, false};
  long long stageSeq = 0; bool directPending = false;   // a DMA may still be reading the page-locked buffer of the last call
  int copyThreads = 8;                  // host threads that move a pageable batch into the pinned slot (GTX_COPY_THREADS)
  DevBuf<u64> out;
  DevBuf<char> scratch;                 // gtxi_scratch
  TextSlot text[2];                     // region text tokenised on the device (gtx_count_add_text): two blocks in flight
  long long textSeq = 0;
  DevBuf<int> textTable; DevBuf<char> textNames; unsigned textMask = 0, textBlobLen = 0;
  std::string textBlob;                               // the chromosome names the device tables were built from

  // scan state
  DevBuf<u64> micro;
  DevBuf<long long> scanTab;
  std::vector<long long> scanKey;       // geometry the tables on the device were built for
  int64_t scanTotalWindows = 0, scanTotalMicro = 0, scanTotalTiles = 0;
  // unsorted reads: bucket tables over the positions of a scan geometry (scan_bucket_tables), the parts they are counted in
  BucketTables bktS; DevBuf<gtx::ScanPart> scanParts; int nScanParts = 0; std::vector<long long> scanBktKey; DevBuf<gtx::DevInfo> scanInfo;
  // owner-computes scan of sorted reads (gtx_scanown.hip): block table for the current tile, bounds scratch, give-up flag;
  // reads of a host-buffer call held resident for its single launch
  int64_t scanOwnBlocks = 0; DevBuf<long long> scanBounds; DevBuf<int> scanFlag;
  DevBuf<char> resReads; DevBuf<int> resWeights; hipEvent_t evRes[2] = {nullptr, nullptr};

  // measurement
  static constexpr int kProfSlots = 64;   // ring: the last 64 profiled calls can be read back
  bool prof = false; long long profCalls = 0;
  int profEvery = 1; long long profSeq = 0; bool profThis = false;   // gtx_profile_enable(N >= 2): kernel-only events on every N-th call
  hipEvent_t evRing[kProfSlots][4] = {};
  hipEvent_t *ev = evRing[0];

  // streaming count (begin/add/end)
  bool streamOpen = false; int64_t streamSeen = 0; int32_t streamLast[2] = {0, 0};
  // gtx_scan_begin .. gtx_scan_end: the open scan's geometry and what its batches have added so far
  struct ScanOpen { bool open = false, weighted = false; gtx::ScanArgs a; std::vector<int32_t> classLen; int64_t extent = 0; char prep = '1'; uint32_t flags = 0;
                    DevBuf<unsigned long long> labelSum; } scan;
  // gtx_scan_end_keep: window vectors that stay in HBM (their extents beside them); the window selection's tile counts and bases,
  // its tables, the total on the host, the host entry's results
  DevBuf<u64> kept[GTX_SCAN_KEEP_SLOTS]; int64_t keptLen[GTX_SCAN_KEEP_SLOTS] = {};
  DevBuf<unsigned> selCount; DevBuf<long long> selBase, selOrd; DevBuf<int> selTab, selRows; PinBuf<long long> selTotal;
  int64_t seamUnsorted = INT64_MAX;    // first order violation found at a seam between batches (host-side check)

  int64_t batchReads = 8ll << 20;       // reads per device batch of the host-buffer entry points (96 MiB of triples: ~2 ms of PCIe)
  int chunksPerWave = 0;                // 0 = choose per call from the number of reads
  int64_t waveSlots = 8192;             // resident waves of the device (CUs x 32)
};

#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return GTX_E_HIP; } } while (0)

static int fail(gtx_ctx *c, int code, const char *msg) { c->err = msg; return code; }

// b = the n elements of v, in a buffer of exactly n
template <class T> static hipError_t upload(DevBuf<T> &b, const T *v, size_t n)
{
  hipError_t e = b.alloc(n);
  return e == hipSuccess ? hipMemcpy(b.get(), v, sizeof(T) * n, hipMemcpyHostToDevice) : e;
}

// histograms, tile sums, prefix arrays, chain flags and tile totals over histLen slots; histograms, tile sums, flags and totals zero
// (the invariant between calls: the finalize kernels leave them so -- of the totals, the ones the next call writes)
static int make_hist_set(gtx_ctx *c, HistSet &h, int64_t histLen)
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
static int make_place_table(gtx_ctx *c, const std::vector<int32_t> &seg, const std::vector<int32_t> &arrA, const std::vector<int32_t> &arrB,
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
static int build_bucket_tables(gtx_ctx *c, BucketTables &t, BucketCuts &k, int nClasses, bool sync = false)
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
  for (auto &slot : c->evRing) for (auto &ev : slot) if (hipEventCreate(&ev) != hipSuccess) { g_create_error = "gtx_create: hipEventCreate failed"; delete c; return nullptr; }
  if (hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking) != hipSuccess) { g_create_error = "gtx_create: hipStreamCreate failed"; delete c; return nullptr; }
  for (int k = 0; k < 2; k++)
    if (hipEventCreateWithFlags(&c->evCopied[k], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->evConsumed[k], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->evRes[k], hipEventDisableTiming) != hipSuccess) {
      g_create_error = "gtx_create: hipEventCreate failed"; delete c; return nullptr;
    }
  { unsigned hc = std::thread::hardware_concurrency(); c->copyThreads = (int)std::max(1u, std::min(hc ? hc : 4u, 8u));
    if (const char *ct = getenv("GTX_COPY_THREADS")) if (atoi(ct) > 0) c->copyThreads = atoi(ct); }
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
  if (c->copyStream) (void)hipStreamSynchronize(c->copyStream);
  for (int k = 0; k < 2; k++)
    for (hipEvent_t e : {c->evCopied[k], c->evConsumed[k], c->evRes[k]}) if (e) (void)hipEventDestroy(e);
  if (c->copyStream) (void)hipStreamDestroy(c->copyStream);
  for (auto &t : c->text) for (hipEvent_t e : {t.evParsed, t.evConsumed, t.evCopied}) if (e) (void)hipEventDestroy(e);
  for (auto &slot : c->evRing) for (auto &ev : slot) if (ev) (void)hipEventDestroy(ev);
  delete c;
}

const char *gtx_last_error(const gtx_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int gtx_set_stream(gtx_ctx *c, void *s) { if (!c) return GTX_E_ARG; c->stream = (hipStream_t)s; return GTX_OK; }

static void adjacent_hand_over(gtx_ctx *c);

int gtx_sync(gtx_ctx *c)
{
  if (!c) return GTX_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->copyStream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->linkPending) {                                              // the last gtx_link_device's info block has arrived
    const gtx::LinkInfo &h = c->linkHost.get()[0];
    c->linkPending->n_groups = h.nGroups; c->linkPending->first_unsorted = h.firstUnsortedOut;
    c->linkPending = nullptr;
  }
  adjacent_hand_over(c);
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

// who counts: any entry point, a group member (its classes only: CountArgs::owned), or a member's call on one of the group's streams
// (gtxi_count_device_share_async)
enum CountCall { COUNT_ANY, COUNT_SHARE, COUNT_SHARE_ASYNC };

// the count kernels' arguments over histogram set h.  hist32: the call is ONE launch of the streaming kernel over unweighted reads
// (a *_device call): 32-bit histogram slots (CountArgs::hist32); the caller hands the same flag to launch_finalize
static gtx::CountArgs count_args(gtx_ctx *c, const HistSet &h, uint32_t flags, int64_t nReads, int64_t indexBase = 0, CountCall who = COUNT_ANY,
                                 bool hist32 = false)
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
static int partition_plan(gtx_ctx *c, const BucketTables &t, int64_t n, int nClasses, bool weighted, gtx::BucketPlan *p, gtx::BucketWork *w, bool *yes)
{
  *yes = false;
  if (t.nB == 0 || !gtx::partition_worth(n, c->bucketMinReads)) return GTX_OK;
  *p = gtx::bucket_plan(n, nClasses, t.nB, t.nCells, weighted);
  if (!(p->pairs < (1ull << 32))) return GTX_OK;
  *yes = true;
  return bucket_scratch(c, *p, t.nB, w);
}

// reads in no particular order: bucket partition + LDS counting for large batches, per-read search kernel otherwise
static int launch_unsorted(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, const gtx::CountArgs &a)
{
  gtx::BucketPlan p; gtx::BucketWork w; bool part;
  { int rc = partition_plan(c, c->ix.bkt, n, a.nClasses, d_weights != nullptr, &p, &w, &part); if (rc) return rc; }
  if (part) HIPCHK(c, gtx::launch_count_bucketed(d_reads, d_weights, n, a, c->ix.bkt.view(), w, p, c->stream));
  else HIPCHK(c, gtx::launch_count(d_reads, d_weights, n, a, false, c->stream));
  return GTX_OK;
}

// Full sorted-merge semantics (GTX_ZERO_LENGTH_OK on a reference set given with GTX_REFS_KEEP_ZERO_LENGTH): intervals with
// start > end + 1 take part by the merge's two comparisons (gtx_special.hip).  Buffers are made on first use.
static int ref_columns(gtx_ctx *c)
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

static int merge_prepare(gtx_ctx *c, uint32_t flags, int mode)
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
static int pairs_batch(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n)
{
  if (c->rx.pairMulti.n > 0) {
    HIPCHK(c, gtx::launch_pair_miss(d_reads, d_weights, n, c->rx.pairMulti.ix, gtx::RegionBlocks{c->rx.blkOf.get(), c->rx.blkIv.get()}, c->rx.pairAcc.get() + c->nRefs, c->stream));
    c->pairUsed = true;
  }
  return GTX_OK;
}

// after the kernels of one batch: the batch against the inverted reference regions
static int merge_batch(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n)
{
  if (c->sideUsed && c->rx.nSpecial) HIPCHK(c, gtx::launch_special_refs(d_reads, d_weights, n, c->rx.specialRefs.get(), c->rx.nSpecial, c->specialMode, c->rx.specialOut.get(), c->stream));
  return GTX_OK;
}

// after the gather: the inverted reads against the other regions, then the inverted regions' sums into their places
static int merge_end(gtx_ctx *c, void *d_out)
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
  c->profThis = c->prof && (c->profEvery <= 1 || (c->profSeq++ % c->profEvery) == 0);
  if (c->profThis) { c->ev = c->evRing[c->profCalls % gtx_ctx::kProfSlots]; HIPCHK(c, hipEventRecord(c->ev[1], c->stream)); }
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
  if (c->profThis) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  rc = count_end(c, d_hits, false, false, h32); if (rc) return rc;
  if (c->profThis) { if (c->profEvery <= 1) HIPCHK(c, hipEventRecord(c->ev[3], c->stream)); c->profCalls++; }
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
static bool is_pinned(const void *p)
{
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

static void parallel_copy(char *dst, const char *src, size_t bytes, int threads)
{
  const int T = (int)std::min<size_t>((size_t)threads, bytes / (4u << 20) + 1);
  if (T <= 1) { memcpy(dst, src, bytes); return; }
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back([=] { const size_t b0 = bytes * (size_t)t / T, b1 = bytes * (size_t)(t + 1) / T; memcpy(dst + b0, src + b0, b1 - b0); });
  memcpy(dst, src, bytes / T);
  for (auto &x : th) x.join();
}

static int stage_reserve(gtx_ctx *c, size_t nReads, bool weights, bool pinnedSlots)
{
  const size_t bytes = nReads * 12, nW = weights ? nReads : 0, pinBytes = pinnedSlots ? nReads * 16 : 0;
  bool grows = false;
  for (int k = 0; k < 2; k++) grows |= bytes > c->stage[k].cap || nW > c->stageW[k].cap || pinBytes > c->pin[k].cap;
  if (grows) {
    // growing: nothing may still be in flight on the old buffers
    HIPCHK(c, hipStreamSynchronize(c->copyStream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->slotBusy[0] = c->slotBusy[1] = false;
  }
  for (int k = 0; k < 2; k++) HIPCHK(c, c->stage[k].reserve(bytes));
  for (int k = 0; k < 2; k++) HIPCHK(c, c->stageW[k].reserve(nW));
  for (int k = 0; k < 2; k++) HIPCHK(c, c->pin[k].reserve(pinBytes));
  return GTX_OK;
}

// Streams reads[0..n) (and weights) through the device in batches; launch(d_reads, d_weights, cnt, off) enqueues the
// kernels of one batch on the context's stream.  Returns with everything enqueued; the caller's buffers are free again
// when the function returns unless they are page-locked, in which case they must stay untouched until the context's next
// host-buffer call, gtx_*_end or gtx_sync has returned.
template <class Launch>
static int stage_batches(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, Launch launch)
{
  if (c->directPending) { HIPCHK(c, hipStreamSynchronize(c->copyStream)); c->directPending = false; }   // the previous call's page-locked source is free now
  if (n <= 0) return GTX_OK;
  const int64_t batch = c->batchReads;
  const bool direct = is_pinned(reads) && (!weights || is_pinned(weights));
  c->directPending = direct;
  int rc = stage_reserve(c, (size_t)std::min<int64_t>(n, batch), weights != nullptr, !direct); if (rc) return rc;
  for (int64_t off = 0; off < n; off += batch) {
    const int64_t cnt = std::min(batch, n - off);
    const int slot = (int)(c->stageSeq++ & 1);
    if (c->slotBusy[slot]) {
      // the pinned slot is free once its DMA is done; the device slot once the kernels that read it are
      if (!direct) HIPCHK(c, hipEventSynchronize(c->evCopied[slot]));
      HIPCHK(c, hipStreamWaitEvent(c->copyStream, c->evConsumed[slot], 0));
    }
    const char *srcR = (const char *)(reads + 3 * off), *srcW = (const char *)(weights ? weights + off : nullptr);
    if (!direct) {
      parallel_copy(c->pin[slot].get(), srcR, (size_t)cnt * 12, c->copyThreads);
      if (weights) parallel_copy(c->pin[slot].get() + (size_t)cnt * 12, srcW, (size_t)cnt * 4, c->copyThreads);
      srcR = c->pin[slot].get(); srcW = c->pin[slot].get() + (size_t)cnt * 12;
    }
    HIPCHK(c, hipMemcpyAsync(c->stage[slot].get(), srcR, (size_t)cnt * 12, hipMemcpyHostToDevice, c->copyStream));
    if (weights) HIPCHK(c, hipMemcpyAsync(c->stageW[slot].get(), srcW, (size_t)cnt * 4, hipMemcpyHostToDevice, c->copyStream));
    HIPCHK(c, hipEventRecord(c->evCopied[slot], c->copyStream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->evCopied[slot], 0));
    rc = launch(c->stage[slot].get(), weights ? c->stageW[slot].get() : nullptr, cnt, off); if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->evConsumed[slot], c->stream));
    c->slotBusy[slot] = true;
  }
  return GTX_OK;
}

extern "C" {

static int ensure_out(gtx_ctx *c, size_t n)
{
  HIPCHK(c, c->out.reserve(n, n + 1));
  return GTX_OK;
}

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
  HIPCHK(c, hipStreamSynchronize(c->copyStream));
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

// the envelopes of the regions `pick` selects, per class in the order of their starts, with the running and the per-64 maxima
// of their ends.  Which regions take part at all follows gtx_set_refs (placeholders and, under the bin index's rules, regions
// with start > stop or stop <= 0 never match); under the sorted merge's rules every region with a class does, inverted or not:
// the envelope test below is the merge's own (CalcDirection == 0, genomic_intervals.cpp:1225-1236).
template <class Pick>
static int build_pair_index(gtx_ctx *c, RefExtras::PairIdx *out, Pick pick)
{
  *out = {};
  struct Item { int32_t cls, s, e, k; };
  std::vector<Item> it;
  for (int64_t k = 0; k < c->nRefs; k++) {
    const int32_t cl = c->h_refC[k], s = c->h_refS[k], e = c->h_refE[k];
    if (cl < 0 || !(c->mergeRefs || !(s > e || e <= 0)) || !pick(k)) continue;
    it.push_back({cl, s, e, (int32_t)k});
  }
  std::sort(it.begin(), it.end(), [](const Item &a, const Item &b) { return a.cls != b.cls ? a.cls < b.cls : (a.s != b.s ? a.s < b.s : a.k < b.k); });
  const size_t n = it.size(), nb = (n + 63) / 64, nc = (size_t)c->nClasses;
  std::vector<int32_t> mem(nc + 1 + 4 * n + nb + 1, 0);
  int32_t *seg = mem.data(), *st = seg + nc + 1, *en = st + n, *pm = en + n, *bm = pm + n, *id = bm + nb;
  for (size_t i = 0; i < n; i++) seg[it[i].cls + 1]++;
  for (size_t cl = 0; cl < nc; cl++) seg[cl + 1] += seg[cl];
  for (size_t i = 0; i < nb; i++) bm[i] = INT32_MIN;
  for (size_t i = 0; i < n; i++) {
    st[i] = it[i].s; en[i] = it[i].e; id[i] = it[i].k;
    pm[i] = (i > 0 && it[i - 1].cls == it[i].cls) ? std::max(pm[i - 1], it[i].e) : it[i].e;
    bm[i >> 6] = std::max(bm[i >> 6], it[i].e);
  }
  HIPCHK(c, upload(out->mem, mem.data(), mem.size()));
  const int *d = out->mem.get();
  out->ix = gtx::PairIndex{d, d + nc + 1, d + nc + 1 + n, d + nc + 1 + 2 * n, d + nc + 1 + 3 * n, d + nc + 1 + 3 * n + nb, c->nClasses};
  out->n = (int)n; out->built = true;
  return GTX_OK;
}

static int pair_acc(gtx_ctx *c)
{
  if (c->rx.pairAcc) return GTX_OK;
  const size_t n = 2 * (size_t)std::max<int64_t>(c->nRefs, 1);
  HIPCHK(c, c->rx.pairAcc.alloc(n));
  HIPCHK(c, hipMemset(c->rx.pairAcc.get(), 0, sizeof(u64) * n));
  return GTX_OK;
}

// {start, stop} lists as the kernels need them: starts and stops both non-decreasing (sorted, disjoint intervals are)
static bool blocks_monotone(const int32_t *b, int64_t cnt)
{
  for (int64_t j = 1; j < cnt; j++) if (b[2 * j] < b[2 * j - 2] || b[2 * j + 1] < b[2 * j - 1]) return false;
  return true;
}

// the reference regions' interval lists as the kernels take them (none: every region is its envelope)
static gtx::RegionBlocks ref_blocks(const gtx_ctx *c) { return gtx::RegionBlocks{c->rx.refBlocks ? c->rx.blkOf.get() : nullptr, c->rx.blkIv.get()}; }

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
// the overlap join (gtx_join.hip)
// ---------------------------------------------------------------------------------------------
} // extern "C"

// the envelope index over all regions, and whether a query's pairs come out of the walk already in key order: the emit pass
// writes them by ascending index position, so that holds when (key, ordinal) ascends along the index inside every class --
// ordinal keys on a position-sorted set (the sorted merge's) are the common case
static int join_prepare(gtx_ctx *c)
{
  if (!c->rx.pairAll.built) { c->rx.joinMono = -1; int rc = build_pair_index(c, &c->rx.pairAll, [](int64_t) { return true; }); if (rc) return rc; }
  if (c->rx.joinMono >= 0) return GTX_OK;
  const int n = c->rx.pairAll.n, nc = c->nClasses;
  std::vector<int32_t> seg(nc + 1), id(std::max(n, 1));
  HIPCHK(c, hipMemcpy(seg.data(), c->rx.pairAll.ix.seg, sizeof(int32_t) * (nc + 1), hipMemcpyDeviceToHost));
  if (n) HIPCHK(c, hipMemcpy(id.data(), c->rx.pairAll.ix.id, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  const bool keyed = !c->rx.h_joinKey.empty();
  bool mono = true;
  for (int cl = 0; cl < nc && mono; cl++)
    for (int i = seg[cl] + 1; i < seg[cl + 1] && mono; i++) {
      const int32_t a = id[i - 1], b = id[i];
      const long long ka = keyed ? c->rx.h_joinKey[a] : a, kb = keyed ? c->rx.h_joinKey[b] : b;
      mono = ka < kb || (ka == kb && a < b);
    }
  c->rx.joinMono = mono ? 1 : 0;
  return GTX_OK;
}

static int join_mode(gtx_ctx *c, uint32_t flags)
{
  return ((flags & GTX_ZERO_LENGTH_OK) ? gtx::JOIN_ZERO_OK : 0) | (c->mergeRefs ? gtx::JOIN_MERGE : 0) |
         ((flags & GTX_CHECK_SORTED) ? gtx::JOIN_CHECK : 0) | ((flags & GTX_JOIN_GAPS) ? gtx::JOIN_GAPS : 0);
}

// count + scan of the n queries into d_off (n + 1 offsets from 0), *total = d_off[n]; info of the count pass in *hi
static int join_count(gtx_ctx *c, const gtx::JoinQueries &q, int mode, long long *d_off, int64_t *total, gtx::JoinInfo *hi)
{
  HIPCHK(c, hipSetDevice(c->device));
  int rc = join_prepare(c); if (rc) return rc;
  if (!c->joinInfo) HIPCHK(c, c->joinInfo.alloc(1));
  if (!c->joinCut) HIPCHK(c, c->joinCut.alloc(2));
  HIPCHK(c, c->joinPart.grow((size_t)gtx::join_scan_partials(q.n + 1)));
  const gtx::JoinInfo init = {0, 0, INT64_MAX, INT64_MAX, 0};
  HIPCHK(c, hipMemcpyAsync(c->joinInfo.get(), &init, sizeof init, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gtx::launch_join_count(q, c->rx.pairAll.ix, ref_blocks(c), mode, d_off, c->joinInfo.get(), c->stream));
  HIPCHK(c, hipMemsetAsync(d_off + q.n, 0, sizeof(long long), c->stream));
  HIPCHK(c, gtx::launch_join_scan(d_off, q.n + 1, c->joinPart.get(), c->stream));
  long long t = 0;
  HIPCHK(c, hipMemcpyAsync(&t, d_off + q.n, sizeof t, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hi, c->joinInfo.get(), sizeof *hi, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *total = t;
  return GTX_OK;
}

// the pairs of queries [q0, q1) into d_pairs (their offsets relative to d_off[q0]), sorted by key; scratch: a buffer as long
static int join_emit(gtx_ctx *c, const gtx::JoinQueries &q, int mode, const long long *d_off, int64_t q0, int64_t q1, int *d_pairs, int *d_scratch)
{
  HIPCHK(c, gtx::launch_join_emit(q, q0, q1, c->rx.pairAll.ix, ref_blocks(c), mode, d_off, d_pairs, c->joinInfo.get(), c->stream));
  if (!c->rx.joinMono) {
    HIPCHK(c, c->joinBig.grow((size_t)(q1 - q0 + 1)));
    HIPCHK(c, gtx::launch_join_sort(d_off, q0, q1, c->rx.joinKey.get(), d_pairs, d_scratch, c->joinBig.get(), c->stream));
  }
  long long mismatch = 0;
  HIPCHK(c, hipMemcpyAsync(&mismatch, &c->joinInfo.get()->mismatch, sizeof mismatch, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (mismatch) return fail(c, GTX_E_HIP, "gtx_join: the emit pass found another number of pairs than the count pass");
  return GTX_OK;
}

// the longest run of queries from q0 whose pairs fit `cap`
static int join_cut(gtx_ctx *c, const long long *d_off, int64_t q0, int64_t n, int64_t cap, int64_t *q1)
{
  HIPCHK(c, gtx::launch_join_cut(d_off, q0, n, cap, c->joinCut.get(), c->stream));
  long long v = 0;
  HIPCHK(c, hipMemcpyAsync(&v, c->joinCut.get(), sizeof v, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *q1 = v;
  return GTX_OK;
}

static void join_info_merge(gtx_count_info *info, const gtx::JoinInfo &h, int64_t base)
{
  info->n_no_class += h.noClass;
  info->n_degenerate += h.degenerate;
  if (h.firstDegenerate != INT64_MAX && info->first_degenerate < 0) info->first_degenerate = h.firstDegenerate + base;
  if (h.firstUnsorted != INT64_MAX && info->first_unsorted < 0) info->first_unsorted = h.firstUnsorted + base;
}

extern "C" {

int gtx_set_ref_order(gtx_ctx *c, const int64_t *key)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_set_ref_order: gtx_set_refs has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rx.joinKey.reset(); c->rx.h_joinKey.clear(); c->rx.joinMono = -1;
  if (!key || c->nRefs == 0) return GTX_OK;
  c->rx.h_joinKey.assign(key, key + c->nRefs);
  HIPCHK(c, upload(c->rx.joinKey, (const long long *)key, (size_t)c->nRefs));
  return GTX_OK;
}

int gtx_set_join_buffer(gtx_ctx *c, int64_t max_pairs)
{
  if (!c) return GTX_E_ARG;
  if (max_pairs < 1) return fail(c, GTX_E_ARG, "gtx_set_join_buffer: at least one pair");
  c->joinBuffer = max_pairs;
  return GTX_OK;
}

int gtx_join_device(gtx_ctx *c, const void *d_reads, int64_t n, uint32_t flags, void *d_offsets, void *d_pairs, int64_t cap,
                    int64_t *n_pairs_out, int64_t *n_done_out, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_join_device: gtx_set_refs has not been called");
  if (n < 0 || (n > 0 && !d_reads) || !d_offsets || cap < 0 || (cap > 0 && !d_pairs)) return fail(c, GTX_E_ARG, "gtx_join_device: bad argument");
  const int mode = join_mode(c, flags);
  const gtx::JoinQueries q{(const int *)d_reads, nullptr, nullptr, n};
  long long *off = (long long *)d_offsets;
  int64_t total = 0; gtx::JoinInfo hi;
  int rc = join_count(c, q, mode, off, &total, &hi); if (rc) return rc;
  int64_t q1 = n;
  if (total > cap) { rc = join_cut(c, off, 0, n, cap, &q1); if (rc) return rc; }
  if (q1 > 0) {
    int64_t len = 0;
    if (q1 < n) HIPCHK(c, hipMemcpy(&len, off + q1, sizeof len, hipMemcpyDeviceToHost)); else len = total;
    if (!c->rx.joinMono) { HIPCHK(c, c->joinScratch.grow((size_t)len)); }
    rc = join_emit(c, q, mode, off, 0, q1, (int *)d_pairs, c->joinScratch.get()); if (rc) return rc;
  }
  if (n_pairs_out) *n_pairs_out = total;
  if (n_done_out) *n_done_out = q1;
  if (info) { memset(info, 0, sizeof *info); info->first_unsorted = -1; info->first_degenerate = -1; join_info_merge(info, hi, 0); }
  return GTX_OK;
}

} // extern "C"

// n host queries as gtx_join takes them: triples, and interval lists (first / blocks) or none
static bool queries_ok(const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t n)
{
  return !(n < 0 || (n > 0 && !reads) || (first && (first[0] != 0 || (first[n] > 0 && !blocks))));
}

// queries [b0, b1) into d_joinReads and q pointed at them; with_blocks: their intervals too (when given) into d_joinQBlk /
// d_joinQIv, checked.  qb / iv hold the host copies until the stream has passed the copies
static int stage_queries(gtx_ctx *c, const std::string &w, const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t b0,
                         int64_t b1, bool with_blocks, std::vector<int2> &qb, std::vector<int2> &iv, gtx::JoinQueries &q)
{
  const int64_t m = b1 - b0;
  HIPCHK(c, c->joinReads.grow((size_t)(3 * m)));
  HIPCHK(c, hipMemcpyAsync(c->joinReads.get(), reads + 3 * b0, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, c->stream));
  q = gtx::JoinQueries{c->joinReads.get(), nullptr, nullptr, m};
  if (!first || !with_blocks) return GTX_OK;
  qb.resize((size_t)m);
  const int64_t i0 = first[b0];
  if (first[b1] - i0 >= INT32_MAX) return fail(c, GTX_E_ARG, (w + ": too many intervals in one batch").c_str());
  for (int64_t i = b0; i < b1; i++) {
    const int64_t cnt = first[i + 1] - first[i];
    if (cnt < 1) return fail(c, GTX_E_ARG, (w + ": every query has at least one interval").c_str());
    const int32_t *b = blocks + 2 * first[i];
    if (b[0] != reads[3 * i + 1] || b[2 * cnt - 1] != reads[3 * i + 2]) return fail(c, GTX_E_ARG, (w + ": a query's triple must be its envelope").c_str());
    if (!blocks_monotone(b, cnt)) return fail(c, GTX_E_RANGE, (w + ": the intervals of a query must be sorted (starts and stops non-decreasing)").c_str());
    qb[i - b0] = make_int2((int)(first[i] - i0), (int)cnt);
  }
  iv.resize((size_t)std::max<int64_t>(first[b1] - i0, 1));
  for (int64_t j = i0; j < first[b1]; j++) iv[j - i0] = make_int2(blocks[2 * j], blocks[2 * j + 1]);
  HIPCHK(c, c->joinQBlk.grow(qb.size()));
  HIPCHK(c, c->joinQIv.grow(iv.size()));
  HIPCHK(c, hipMemcpyAsync(c->joinQBlk.get(), qb.data(), sizeof(int2) * qb.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->joinQIv.get(), iv.data(), sizeof(int2) * iv.size(), hipMemcpyHostToDevice, c->stream));
  q.blk = c->joinQBlk.get(); q.iv = c->joinQIv.get();
  return GTX_OK;
}

// the body of gtx_join / gtx_join_offsets: the queries in batches of batchReads, the pairs of each batch in chunks of at most
// joinBuffer pairs.  on_chunk(q, b0, q0, q1, p0, len) runs when the pairs of the batch's queries [q0, q1) are in d_joinPairs (their
// offsets relative to d_joinOff[q0]; p0: the position of the first among all pairs).  all_blocks: the queries' intervals go to
// the device under GTX_JOIN_GAPS too.
typedef std::function<int(const gtx::JoinQueries &, int64_t, int64_t, int64_t, int64_t, int64_t)> JoinChunk;
static int join_batches(gtx_ctx *c, const char *who, const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t n, uint32_t flags,
                        bool all_blocks, int64_t *offsets_out, int64_t cap, gtx_count_info *info, const JoinChunk &on_chunk)
{
  const std::string w(who);
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, (w + ": gtx_set_refs has not been called").c_str());
  if (!offsets_out || cap < 0 || !queries_ok(reads, first, blocks, n)) return fail(c, GTX_E_ARG, (w + ": bad argument").c_str());
  HIPCHK(c, hipSetDevice(c->device));
  const int mode = join_mode(c, flags);
  gtx_count_info acc; memset(&acc, 0, sizeof acc); acc.first_unsorted = -1; acc.first_degenerate = -1;
  int64_t base = 0;                                            // pairs before the batch
  offsets_out[0] = 0;
  const int64_t per = std::max<int64_t>(1, c->batchReads);
  for (int64_t b0 = 0; b0 < n; b0 += per) {
    const int64_t b1 = std::min(n, b0 + per), m = b1 - b0;
    gtx::JoinQueries q{};
    std::vector<int2> qb, iv;
    int rc = stage_queries(c, w, reads, first, blocks, b0, b1, all_blocks || !(mode & gtx::JOIN_GAPS), qb, iv, q); if (rc) return rc;
    HIPCHK(c, c->joinOff.grow((size_t)(m + 1)));
    int64_t total = 0; gtx::JoinInfo hi;
    rc = join_count(c, q, mode, c->joinOff.get(), &total, &hi); if (rc) return rc;      // (synchronises: qb / iv may go)
    if ((flags & GTX_CHECK_SORTED) && b0 > 0 && acc.first_unsorted < 0) {           // the seam between two batches comes before the batch's own
      const int32_t *p = reads + 3 * (b0 - 1), *r = reads + 3 * b0;
      if (r[0] < p[0] || (r[0] == p[0] && r[1] < p[1])) acc.first_unsorted = b0;
    }
    join_info_merge(&acc, hi, b0);
    HIPCHK(c, hipMemcpy(offsets_out + b0, c->joinOff.get(), sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost));
    for (int64_t i = b0; i <= b1; i++) offsets_out[i] += base;
    // pairs chunk by chunk: the longest run of queries that fits the device buffer, or one query alone in a buffer of its size
    const int64_t chunk = std::min<int64_t>(c->joinBuffer, std::max<int64_t>(total, 1));
    for (int64_t q0 = 0; q0 < m && offsets_out[b0 + q0] < cap;) {
      int64_t q1 = m;
      if (offsets_out[b1] - offsets_out[b0 + q0] > chunk) { rc = join_cut(c, c->joinOff.get(), q0, m, chunk, &q1); if (rc) return rc; }
      if (q1 == q0) q1 = q0 + 1;
      const int64_t p0 = offsets_out[b0 + q0], len = offsets_out[b0 + q1] - p0;
      if (len > 0) {
        HIPCHK(c, c->joinPairs.grow((size_t)len));
        if (!c->rx.joinMono) { HIPCHK(c, c->joinScratch.grow((size_t)len)); }
        rc = join_emit(c, q, mode, c->joinOff.get(), q0, q1, c->joinPairs.get(), c->joinScratch.get()); if (rc) return rc;
        rc = on_chunk(q, b0, q0, q1, p0, len); if (rc) return rc;
      }
      q0 = q1;
    }
    base = offsets_out[b1];
  }
  if (info) *info = acc;
  return GTX_OK;
}

extern "C" {

int gtx_join(gtx_ctx *c, const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t n, uint32_t flags,
             int64_t *offsets_out, int32_t *pairs_out, int64_t cap, gtx_count_info *info)
{
  if (c && c->nRefs >= 0 && cap > 0 && !pairs_out) return fail(c, GTX_E_ARG, "gtx_join: bad argument");
  return join_batches(c, "gtx_join", reads, first, blocks, n, flags, false, offsets_out, cap, info,
                      [&](const gtx::JoinQueries &, int64_t, int64_t, int64_t, int64_t p0, int64_t len) {
                        const int64_t keep = std::min(len, cap - p0);
                        HIPCHK(c, hipMemcpy(pairs_out + p0, c->joinPairs.get(), sizeof(int32_t) * keep, hipMemcpyDeviceToHost));
                        return GTX_OK;
                      });
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// per-query hits (gtx_query.hip)
// ---------------------------------------------------------------------------------------------

// d_hits[i] = the pairs of query i, *hi = what the pass observed: the join's count walk, its counts narrowed to 32 bits.  Returns
// with the work complete.
static int hits_pass(gtx_ctx *c, const gtx::JoinQueries &q, int mode, unsigned *d_hits, gtx::JoinInfo *hi)
{
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->joinInfo) HIPCHK(c, c->joinInfo.alloc(1));
  const gtx::JoinInfo init = {0, 0, INT64_MAX, INT64_MAX, 0};
  *hi = init;
  if (q.n == 0) return GTX_OK;
  HIPCHK(c, hipMemcpyAsync(c->joinInfo.get(), &init, sizeof init, hipMemcpyHostToDevice, c->stream));
  int rc = join_prepare(c); if (rc) return rc;
  HIPCHK(c, c->joinOff.grow((size_t)q.n));
  HIPCHK(c, gtx::launch_join_count(q, c->rx.pairAll.ix, ref_blocks(c), mode, c->joinOff.get(), c->joinInfo.get(), c->stream));
  HIPCHK(c, gtx::launch_query_narrow(c->joinOff.get(), q.n, d_hits, c->stream));
  HIPCHK(c, hipMemcpyAsync(hi, c->joinInfo.get(), sizeof *hi, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTX_OK;
}

extern "C" {

int gtx_query_hits_device(gtx_ctx *c, const void *d_reads, int64_t n, uint32_t flags, void *d_hits, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_query_hits_device: gtx_set_refs has not been called");
  if (n < 0 || (n > 0 && (!d_reads || !d_hits))) return fail(c, GTX_E_ARG, "gtx_query_hits_device: bad argument");
  const int mode = join_mode(c, flags);
  const gtx::JoinQueries q{(const int *)d_reads, nullptr, nullptr, n};
  gtx::JoinInfo hi;
  int rc = hits_pass(c, q, mode, (unsigned *)d_hits, &hi); if (rc) return rc;
  if (info) { memset(info, 0, sizeof *info); info->first_unsorted = -1; info->first_degenerate = -1; join_info_merge(info, hi, 0); }
  return GTX_OK;
}

int gtx_query_hits(gtx_ctx *c, const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t n, uint32_t flags,
                   uint32_t *hits_out, gtx_count_info *info)
{
  const std::string w("gtx_query_hits");
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_query_hits: gtx_set_refs has not been called");
  if ((n > 0 && !hits_out) || !queries_ok(reads, first, blocks, n)) return fail(c, GTX_E_ARG, "gtx_query_hits: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  const int mode = join_mode(c, flags);
  const bool with_blocks = first && !(mode & gtx::JOIN_GAPS);   // (under -gaps the envelopes alone decide)
  gtx_count_info acc; memset(&acc, 0, sizeof acc); acc.first_unsorted = -1; acc.first_degenerate = -1;
  const int64_t per = std::max<int64_t>(1, c->batchReads);
  for (int64_t b0 = 0; b0 < n; b0 += per) {
    const int64_t b1 = std::min(n, b0 + per), m = b1 - b0;
    gtx::JoinQueries q{};
    std::vector<int2> qb, iv;
    int rc = stage_queries(c, w, reads, first, blocks, b0, b1, with_blocks, qb, iv, q); if (rc) return rc;
    HIPCHK(c, c->hitsOut.grow((size_t)m));
    gtx::JoinInfo hi;
    rc = hits_pass(c, q, mode, c->hitsOut.get(), &hi); if (rc) return rc;                 // (synchronises: qb / iv may go)
    if ((flags & GTX_CHECK_SORTED) && b0 > 0 && acc.first_unsorted < 0) {                         // the seam between two batches, as in join_batches
      const int32_t *p = reads + 3 * (b0 - 1), *r = reads + 3 * b0;
      if (r[0] < p[0] || (r[0] == p[0] && r[1] < p[1])) acc.first_unsorted = b0;
    }
    join_info_merge(&acc, hi, b0);
    HIPCHK(c, hipMemcpy(hits_out + b0, c->hitsOut.get(), sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
  }
  if (info) *info = acc;
  return GTX_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// pair offsets (gtx_offset.hip)
// ---------------------------------------------------------------------------------------------

// the per-ordinal reference point (front / back interval) as of gtx_set_ref_blocks
static int offset_prepare(gtx_ctx *c)
{
  if (c->rx.offRef) return GTX_OK;
  const size_t m = (size_t)std::max<int64_t>(c->nRefs, 1);
  std::vector<int2> env(m, make_int2(0, 0));
  for (int64_t k = 0; k < c->nRefs; k++) env[k] = make_int2(c->h_refS[k], c->h_refE[k]);
  DevBuf<int2> d_env;
  HIPCHK(c, d_env.alloc(m));
  HIPCHK(c, c->rx.offRef.alloc(m));
  HIPCHK(c, hipMemcpy(d_env.get(), env.data(), sizeof(int2) * m, hipMemcpyHostToDevice));
  HIPCHK(c, gtx::launch_ref_ends(d_env.get(), ref_blocks(c), c->nRefs, c->rx.offRef.get(), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));                   // (before d_env goes)
  return GTX_OK;
}

static int offset_op(int32_t op) { return op >= GTX_OFFSET_1 && op <= GTX_OFFSET_3P ? op : 0; }

// the offsets of the pairs of queries [q0, q1) into d_out; *inv = the first inverted pair (relative to d_off[q0]), INT64_MAX if none.
// Waits for the stream.
static int pair_offsets(gtx_ctx *c, const gtx::OffsetArgs &a, int64_t q0, int64_t q1, const long long *d_off, const int *d_pairs, int64_t n_pairs,
                        long long *d_out, long long *inv)
{
  const long long none = INT64_MAX;
  HIPCHK(c, hipMemcpyAsync(c->offInv.get(), &none, sizeof none, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gtx::launch_pair_offsets(a, q0, q1, d_off, d_pairs, n_pairs, d_out, c->offInv.get(), c->joinBig.get(), c->stream));
  *inv = INT64_MAX;
  HIPCHK(c, hipMemcpyAsync(inv, c->offInv.get(), sizeof *inv, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTX_OK;
}

extern "C" {

int gtx_set_ref_strands(gtx_ctx *c, const int8_t *strand)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_set_ref_strands: gtx_set_refs has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rx.refStrand.reset();
  if (!strand || c->nRefs == 0) return GTX_OK;
  for (int64_t k = 0; k < c->nRefs; k++)
    if (strand[k] != '+' && strand[k] != '-') return fail(c, GTX_E_ARG, "gtx_set_ref_strands: a strand is '+' or '-'");
  HIPCHK(c, upload(c->rx.refStrand, strand, (size_t)c->nRefs));
  return GTX_OK;
}

int gtx_join_offsets(gtx_ctx *c, const int32_t *reads, const int64_t *first, const int32_t *blocks, const int8_t *read_strands, int64_t n,
                     uint32_t flags, int32_t op, int64_t *offsets_out, int32_t *pairs_out, int64_t cap, int64_t *entry_offsets_out,
                     int64_t *entries_out, int64_t entry_cap, int64_t *first_inverted_out, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_join_offsets: gtx_set_refs has not been called");
  const int o = offset_op(op);
  const bool skip = flags & GTX_OFFSET_SKIP_REF_GAPS, fromQuery = flags & GTX_OFFSET_FROM_QUERY;
  if (!o || (skip && fromQuery) || cap < 0 || (cap > 0 && (!pairs_out || !entry_offsets_out)) || entry_cap < 0 || (entry_cap > 0 && !entries_out))
    return fail(c, GTX_E_ARG, "gtx_join_offsets: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = offset_prepare(c); if (rc) return rc;
  int64_t ebase = 0, inverted = -1, strandsOf = -1;            // entries before the chunk; the first inverted pair; the batch whose strands are up
  if (cap > 0) entry_offsets_out[0] = 0;
  if (!c->offInv) HIPCHK(c, c->offInv.alloc(1));
  rc = join_batches(c, "gtx_join_offsets", reads, first, blocks, n, flags, true, offsets_out, cap, info,
    [&](const gtx::JoinQueries &q, int64_t b0, int64_t q0, int64_t q1, int64_t p0, int64_t len) -> int {
      int r = GTX_OK;
      const int64_t keep = std::min(len, cap - p0);
      HIPCHK(c, hipMemcpy(pairs_out + p0, c->joinPairs.get(), sizeof(int32_t) * keep, hipMemcpyDeviceToHost));
      gtx::OffsetArgs a{q, nullptr, c->rx.offRef.get(), c->rx.refStrand.get(), ref_blocks(c), o, fromQuery};
      if (fromQuery && read_strands) {
        if (strandsOf != b0) {
          const int64_t m = std::min<int64_t>(n - b0, std::max<int64_t>(1, c->batchReads));
          HIPCHK(c, c->offQStrand.grow((size_t)m));
          HIPCHK(c, hipMemcpy(c->offQStrand.get(), read_strands + b0, (size_t)m, hipMemcpyHostToDevice));
          strandsOf = b0;
        }
        a.qStrand = c->offQStrand.get();
      }
      HIPCHK(c, c->joinBig.grow((size_t)(q1 - q0 + 1)));
      int64_t nent = len;
      if (!skip) {
        HIPCHK(c, c->offOut.grow((size_t)(2 * len)));
        long long inv;
        r = pair_offsets(c, a, q0, q1, c->joinOff.get(), c->joinPairs.get(), len, c->offOut.get(), &inv); if (r) return r;
        if (inverted < 0 && inv < keep) inverted = p0 + inv;
        for (int64_t p = 1; p <= keep; p++) entry_offsets_out[p0 + p] = ebase + p;
        nent = keep;
      } else {
        HIPCHK(c, c->offCnt.grow((size_t)(len + 1)));
        HIPCHK(c, c->offPart.grow((size_t)gtx::join_scan_partials(len + 1)));
        HIPCHK(c, gtx::launch_pair_gaps_count(a, q0, q1, c->joinOff.get(), c->joinPairs.get(), len, c->offCnt.get(), c->joinBig.get(), c->stream));
        HIPCHK(c, hipMemsetAsync(c->offCnt.get() + len, 0, sizeof(long long), c->stream));
        HIPCHK(c, gtx::launch_join_scan(c->offCnt.get(), len + 1, c->offPart.get(), c->stream));
        std::vector<int64_t> eoff((size_t)len + 1);
        HIPCHK(c, hipMemcpyAsync(eoff.data(), c->offCnt.get(), sizeof(int64_t) * (len + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nent = eoff[len];
        HIPCHK(c, c->offOut.grow((size_t)(2 * nent)));
        if (nent > 0) HIPCHK(c, gtx::launch_pair_gaps_emit(a, q0, q1, c->joinOff.get(), c->joinPairs.get(), len, c->offCnt.get(), c->offOut.get(), c->joinBig.get(), c->stream));
        for (int64_t p = 1; p <= keep; p++) entry_offsets_out[p0 + p] = ebase + eoff[p];
        nent = eoff[keep];
      }
      const int64_t ekeep = std::max<int64_t>(0, std::min(nent, entry_cap - ebase));
      if (ekeep > 0) HIPCHK(c, hipMemcpy(entries_out + 2 * ebase, c->offOut.get(), sizeof(int64_t) * 2 * ekeep, hipMemcpyDeviceToHost));
      ebase += nent;
      return GTX_OK;
    });
  if (rc) return rc;
  if (first_inverted_out) *first_inverted_out = inverted;
  return GTX_OK;
}

int gtx_pair_offsets_device(gtx_ctx *c, const void *d_reads, int64_t n, const void *d_offsets, const void *d_pairs, int64_t n_pairs, int32_t op,
                            void *d_out, int64_t *first_inverted_out)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_pair_offsets_device: gtx_set_refs has not been called");
  const int o = offset_op(op);
  if (!o || n < 0 || (n > 0 && (!d_reads || !d_offsets)) || n_pairs < 0 || (n_pairs > 0 && (!d_pairs || !d_out)))
    return fail(c, GTX_E_ARG, "gtx_pair_offsets_device: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = offset_prepare(c); if (rc) return rc;
  if (!c->offInv) HIPCHK(c, c->offInv.alloc(1));
  HIPCHK(c, c->joinBig.grow((size_t)(n + 1)));
  const gtx::OffsetArgs a{gtx::JoinQueries{(const int *)d_reads, nullptr, nullptr, n}, nullptr, c->rx.offRef.get(), c->rx.refStrand.get(), ref_blocks(c), o, false};
  long long inv;
  rc = pair_offsets(c, a, 0, n, (const long long *)d_offsets, (const int *)d_pairs, n_pairs, (long long *)d_out, &inv); if (rc) return rc;
  if (first_inverted_out) *first_inverted_out = inv == INT64_MAX ? -1 : inv;
  return GTX_OK;
}

// ---- the annotate pass (gtx_annotate.hip) ----

} // extern "C"

static bool annotate_args(gtx_ctx *c, int64_t n_primary, int32_t op_primary, int32_t op_rest, int32_t mode, const int *d_tri, gtx::AnnotateArgs *a)
{
  if (!offset_op(op_primary) || !offset_op(op_rest) || n_primary < 0 || n_primary > c->nRefs || (mode != GTX_ANNOTATE_CENTER && mode != GTX_ANNOTATE_START)) return false;
  *a = gtx::AnnotateArgs{d_tri, c->rx.offRef.get(), c->rx.refStrand.get(), c->nRefs, n_primary, op_primary, op_rest,
                         mode == GTX_ANNOTATE_CENTER ? gtx::ANN_CENTER : gtx::ANN_START};
  return true;
}

// count, scan and emit over the pairs of queries [q0, q1): d_cnt (q1 - q0 + 1) becomes the kept offsets from 0, *kept their total;
// the kept pairs below cap go to d_ref / d_val.  Waits for the stream.
static int annotate_pass(gtx_ctx *c, const gtx::AnnotateArgs &a, int64_t q0, int64_t q1, const long long *d_off, const int *d_pairs, int64_t n_pairs,
                         long long *d_cnt, int *d_ref, long long *d_val, int64_t cap, int64_t *kept)
{
  const int64_t m = q1 - q0;
  HIPCHK(c, c->joinBig.grow((size_t)(m + 1)));
  HIPCHK(c, c->offPart.grow((size_t)gtx::join_scan_partials(m + 1)));
  HIPCHK(c, gtx::launch_annotate_count(a, q0, q1, d_off, d_pairs, n_pairs, d_cnt, c->joinBig.get(), c->stream));
  HIPCHK(c, hipMemsetAsync(d_cnt + m, 0, sizeof(long long), c->stream));
  HIPCHK(c, gtx::launch_join_scan(d_cnt, m + 1, c->offPart.get(), c->stream));
  HIPCHK(c, gtx::launch_annotate_emit(a, q0, q1, d_off, d_pairs, n_pairs, d_cnt, d_ref, d_val, cap, c->joinBig.get(), c->stream));
  long long t = 0;
  HIPCHK(c, hipMemcpyAsync(&t, d_cnt + m, sizeof t, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *kept = t;
  return GTX_OK;
}

extern "C" {

int gtx_pair_annotate_device(gtx_ctx *c, const void *d_reads, int64_t n, const void *d_offsets, const void *d_pairs, int64_t n_pairs, int64_t n_primary,
                             int32_t op_primary, int32_t op_rest, int32_t mode, void *d_kept_offsets, void *d_kept_ref, void *d_kept_value,
                             int64_t cap, int64_t *n_kept_out)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_pair_annotate_device: gtx_set_refs has not been called");
  gtx::AnnotateArgs a;
  if (n < 0 || !d_kept_offsets || (n > 0 && (!d_reads || !d_offsets)) || n_pairs < 0 || (n_pairs > 0 && !d_pairs) || cap < 0 ||
      (cap > 0 && (!d_kept_ref || !d_kept_value)) || !annotate_args(c, n_primary, op_primary, op_rest, mode, (const int *)d_reads, &a))
    return fail(c, GTX_E_ARG, "gtx_pair_annotate_device: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = offset_prepare(c); if (rc) return rc;
  a.refEnds = c->rx.offRef.get();
  int64_t kept = 0;
  if (n == 0) HIPCHK(c, hipMemsetAsync(d_kept_offsets, 0, sizeof(long long), c->stream));
  rc = annotate_pass(c, a, 0, n, (const long long *)d_offsets, (const int *)d_pairs, n_pairs, (long long *)d_kept_offsets, (int *)d_kept_ref,
                     (long long *)d_kept_value, cap, &kept); if (rc) return rc;
  if (n_kept_out) *n_kept_out = kept;
  return GTX_OK;
}

int gtx_join_annotate(gtx_ctx *c, const int32_t *reads, int64_t n, uint32_t flags, int64_t n_primary, int32_t op_primary, int32_t op_rest, int32_t mode,
                      int64_t *kept_offsets_out, int32_t *kept_ref_out, int64_t *kept_value_out, int64_t cap, int64_t *n_pairs_out, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_join_annotate: gtx_set_refs has not been called");
  gtx::AnnotateArgs a;
  if (!kept_offsets_out || cap < 0 || (cap > 0 && (!kept_ref_out || !kept_value_out)) || !annotate_args(c, n_primary, op_primary, op_rest, mode, nullptr, &a))
    return fail(c, GTX_E_ARG, "gtx_join_annotate: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = offset_prepare(c); if (rc) return rc;
  a.refEnds = c->rx.offRef.get();
  std::vector<int64_t> off((size_t)std::max<int64_t>(n, 0) + 1, 0), koff;
  int64_t kbase = 0, done = 0;                                 // kept pairs before the chunk; queries whose kept offsets are written
  kept_offsets_out[0] = 0;
  rc = join_batches(c, "gtx_join_annotate", reads, nullptr, nullptr, n, flags, false, off.data(), INT64_MAX, info,
    [&](const gtx::JoinQueries &q, int64_t b0, int64_t q0, int64_t q1, int64_t, int64_t len) -> int {
      const int64_t m = q1 - q0;
      for (; done < b0 + q0; done++) kept_offsets_out[done + 1] = kbase;      // (queries in front of the chunk that had no pair)
      a.tri = q.tri;
      const int64_t room = std::max<int64_t>(0, std::min(len, cap - kbase));
      HIPCHK(c, c->annCnt.grow((size_t)(m + 1)));
      HIPCHK(c, c->annRef.grow((size_t)std::max<int64_t>(room, 1)));
      HIPCHK(c, c->annVal.grow((size_t)std::max<int64_t>(room, 1)));
      int64_t kept = 0;
      int r = annotate_pass(c, a, q0, q1, c->joinOff.get(), c->joinPairs.get(), len, c->annCnt.get(), c->annRef.get(), c->annVal.get(), room, &kept);
      if (r) return r;
      koff.resize((size_t)m + 1);
      HIPCHK(c, hipMemcpy(koff.data(), c->annCnt.get(), sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost));
      for (int64_t i = 1; i <= m; i++) kept_offsets_out[b0 + q0 + i] = kbase + koff[i];
      done = b0 + q1;
      const int64_t take = std::min(kept, room);
      if (take > 0) {
        HIPCHK(c, hipMemcpy(kept_ref_out + kbase, c->annRef.get(), sizeof(int32_t) * take, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(kept_value_out + kbase, c->annVal.get(), sizeof(int64_t) * take, hipMemcpyDeviceToHost));
      }
      kbase += kept;
      return GTX_OK;
    });
  if (rc) return rc;
  for (; done < n; done++) kept_offsets_out[done + 1] = kbase;
  if (n_pairs_out) *n_pairs_out = off[(size_t)std::max<int64_t>(n, 0)];
  return GTX_OK;
}

int gtx_set_signal_bins(gtx_ctx *c, double bin_min, double bin_max, int64_t n_bins, const int64_t *ref_len)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_set_signal_bins: gtx_set_refs has not been called");
  if (n_bins < 0 || n_bins >= INT32_MAX) return fail(c, GTX_E_ARG, "gtx_set_signal_bins: n_bins must lie in [0, 2^31 - 1)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rx.sigRefLen.reset();
  if (ref_len && c->nRefs > 0) HIPCHK(c, upload(c->rx.sigRefLen, (const long long *)ref_len, (size_t)c->nRefs));
  c->rx.sigMin = bin_min; c->rx.sigMax = bin_max; c->rx.sigBins = n_bins; c->rx.sigSet = true;
  return GTX_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// signal bins (gtx_signal.hip)
// ---------------------------------------------------------------------------------------------

static const uint32_t kSignalFlags = GTX_ZERO_LENGTH_OK | GTX_JOIN_GAPS | GTX_SIGNAL_PER_REF | GTX_READS_SORTED | GTX_READS_UNSORTED;

// the index, the reference points and the info block of a call; a = everything but the reads and their weights
static int signal_prepare(gtx_ctx *c, const char *who, uint32_t flags, gtx::SignalArgs &a)
{
  const std::string w(who);
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, (w + ": gtx_set_refs has not been called").c_str());
  if (!c->rx.sigSet) return fail(c, GTX_E_STATE, (w + ": gtx_set_signal_bins has not been called").c_str());
  if (flags & ~kSignalFlags) return fail(c, GTX_E_ARG, (w + ": unknown flag").c_str());
  HIPCHK(c, hipSetDevice(c->device));
  int rc = join_prepare(c); if (rc) return rc;
  rc = offset_prepare(c); if (rc) return rc;
  if (!c->sigInfo) HIPCHK(c, c->sigInfo.alloc(1));
  a = gtx::SignalArgs{};
  a.ix = c->rx.pairAll.ix;
  a.rb = ref_blocks(c);
  a.mode = join_mode(c, flags & (GTX_ZERO_LENGTH_OK | GTX_JOIN_GAPS));
  a.refEnds = c->rx.offRef.get(); a.refStrand = (const signed char *)c->rx.refStrand.get(); a.refLen = c->rx.sigRefLen.get();
  a.binMin = c->rx.sigMin; a.binMax = c->rx.sigMax; a.nBins = c->rx.sigBins;
  a.perRef = (flags & GTX_SIGNAL_PER_REF) != 0;
  return GTX_OK;
}

static int64_t signal_len(const gtx_ctx *c, uint32_t flags) { return ((flags & GTX_SIGNAL_PER_REF) ? std::max<int64_t>(c->nRefs, 0) : 1) * c->rx.sigBins; }
static int signal_cus(const gtx_ctx *c) { return (int)std::max<int64_t>(1, c->waveSlots / 32); }

// the signal pass of a.q into d_bins with a fresh info block, then that block into *info / *firstInv (read indices from base);
// waits for the stream
static int signal_pass(gtx_ctx *c, const gtx::SignalArgs &a, unsigned long long *d_bins, gtx_signal_info *info, long long *firstInv, int64_t base)
{
  const gtx::SignalInfo init = {0, 0, 0, 0, 0, 0, INT64_MAX};
  HIPCHK(c, hipMemcpyAsync(c->sigInfo.get(), &init, sizeof init, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gtx::launch_signal_bins(a, d_bins, c->sigInfo.get(), signal_cus(c), c->stream));
  gtx::SignalInfo h;
  HIPCHK(c, hipMemcpyAsync(&h, c->sigInfo.get(), sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (info) {
    info->n_pairs += (int64_t)h.pairs; info->n_binned += (int64_t)h.binned; info->n_dropped += (int64_t)h.dropped;
    info->weight_abs_sum += (int64_t)h.absWeight; info->n_no_class += (int64_t)h.noClass; info->n_degenerate += (int64_t)h.degenerate;
  }
  if (h.firstInverted != INT64_MAX && *firstInv < 0) *firstInv = h.firstInverted + base;
  return GTX_OK;
}

extern "C" {

int gtx_signal_bins_device(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, uint32_t flags, void *d_bins,
                           int64_t *first_inverted_out, gtx_signal_info *info)
{
  if (!c) return GTX_E_ARG;
  gtx::SignalArgs a;
  int rc = signal_prepare(c, "gtx_signal_bins_device", flags, a); if (rc) return rc;
  if (n < 0 || (n > 0 && !d_reads) || (signal_len(c, flags) > 0 && !d_bins)) return fail(c, GTX_E_ARG, "gtx_signal_bins_device: bad argument");
  a.q = gtx::JoinQueries{(const int *)d_reads, nullptr, nullptr, n};
  a.w = (const long long *)d_weights;
  if (info) memset(info, 0, sizeof *info);
  long long inv = -1;
  rc = signal_pass(c, a, (unsigned long long *)d_bins, info, &inv, 0); if (rc) return rc;
  if (first_inverted_out) *first_inverted_out = inv;
  return GTX_OK;
}

int gtx_signal_bins(gtx_ctx *c, const int32_t *reads, const int64_t *first, const int32_t *blocks, const int64_t *weights, int64_t n,
                    uint32_t flags, int64_t *bins_out, int64_t *first_inverted_out, gtx_signal_info *info)
{
  if (!c) return GTX_E_ARG;
  gtx::SignalArgs a;
  int rc = signal_prepare(c, "gtx_signal_bins", flags, a); if (rc) return rc;
  const int64_t len = signal_len(c, flags);
  if ((len > 0 && !bins_out) || !queries_ok(reads, first, blocks, n)) return fail(c, GTX_E_ARG, "gtx_signal_bins: bad argument");
  if (info) memset(info, 0, sizeof *info);
  HIPCHK(c, c->sigBins.grow((size_t)std::max<int64_t>(len, 1)));
  HIPCHK(c, hipMemsetAsync(c->sigBins.get(), 0, sizeof(unsigned long long) * (size_t)std::max<int64_t>(len, 1), c->stream));
  long long inv = -1;
  const int64_t per = std::max<int64_t>(1, c->batchReads);
  const std::string who("gtx_signal_bins");
  for (int64_t b0 = 0; b0 < n; b0 += per) {
    const int64_t b1 = std::min(n, b0 + per), m = b1 - b0;
    std::vector<int2> qb, iv;
    rc = stage_queries(c, who, reads, first, blocks, b0, b1, true, qb, iv, a.q); if (rc) return rc;
    a.w = nullptr;
    if (weights) {
      HIPCHK(c, c->sigW.grow((size_t)m));
      HIPCHK(c, hipMemcpyAsync(c->sigW.get(), weights + b0, sizeof(int64_t) * m, hipMemcpyHostToDevice, c->stream));
      a.w = c->sigW.get();
    }
    rc = signal_pass(c, a, c->sigBins.get(), info, &inv, b0); if (rc) return rc;          // (synchronises: qb / iv may go)
  }
  if (len > 0) {
    std::vector<int64_t> h((size_t)len);
    HIPCHK(c, hipMemcpy(h.data(), c->sigBins.get(), sizeof(int64_t) * (size_t)len, hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < len; k++) bins_out[k] = (int64_t)((uint64_t)bins_out[k] + (uint64_t)h[k]);
  }
  if (first_inverted_out) *first_inverted_out = inv;
  return GTX_OK;
}

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

// One batch of reads into the four coverage histograms: the streaming kernel (exact for any order, fast for sorted reads), or --
// for a batch the caller (GTX_READS_UNSORTED) or a sample of the host buffer says is in no particular order -- the partition path.
static int cover_launch(gtx_ctx *c, const void *dR, const int *dW, int64_t n, int64_t indexBase, uint32_t flags, bool unsorted)
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
static bool host_reads_look_unsorted(const int32_t *tri, int64_t n)
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
  c->profThis = c->prof && (c->profEvery <= 1 || (c->profSeq++ % c->profEvery) == 0);
  if (c->profThis) { c->ev = c->evRing[c->profCalls % gtx_ctx::kProfSlots]; HIPCHK(c, hipEventRecord(c->ev[1], c->stream)); }
  if (flags & GTX_GAPS_FORMULA) { rc = merge_prepare(c, flags, 2); if (rc) return rc; }
  rc = cover_launch(c, d_reads, (const int *)d_weights, n, 0, flags, (flags & GTX_READS_UNSORTED) != 0); if (rc) return rc;
  rc = merge_batch(c, d_reads, d_weights, n); if (rc) return rc;
  if (c->profThis) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  rc = cover_end(c, d_cov); if (rc) return rc;
  if (c->profThis) { if (c->profEvery <= 1) HIPCHK(c, hipEventRecord(c->ev[3], c->stream)); c->profCalls++; }
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
  HIPCHK(c, hipStreamSynchronize(c->copyStream));
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
  if (key != c->scanKey) {
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
    c->scanTotalTiles = to; c->scanOwnBlocks = bo;
    HIPCHK(c, c->scanTab.reserve(tabLen));
    HIPCHK(c, c->micro.reserve((size_t)mo + 1, (size_t)mo + 3));
    HIPCHK(c, c->scanBounds.reserve((size_t)(2 * bo + 2)));
    if (!c->scanFlag) HIPCHK(c, c->scanFlag.alloc(1));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->scanTab.get(), tab.data(), tabLen * sizeof(long long), hipMemcpyHostToDevice));
    c->scanKey = key; c->scanTotalMicro = mo; c->scanTotalWindows = wo;
  }
  out->micro = c->micro.get(); out->microOff = c->scanTab.get(); out->nMicro = c->scanTab.get() + nClasses;
  out->winOff = c->scanTab.get() + 2 * nClasses; out->outOff = c->scanTab.get() + 3 * nClasses + 1; out->tileOff = c->scanTab.get() + 4 * nClasses + 1;
  out->nClasses = nClasses; out->winStep = step; out->comb = size / step;
  out->winStepInv = step > 1 ? (unsigned)((1ull << 32) / (unsigned)step) : 0;
  if (own) { own->blkOff = c->scanTab.get() + 5 * nClasses + 2; own->tile = ownTile; own->totalBlocks = c->scanOwnBlocks; own->bounds = c->scanBounds.get(); own->flag = c->scanFlag.get(); }
  return GTX_OK;
}

// Bucket tables over the POSITIONS of a scan geometry, for reads in no particular order (gtx_bucket.hip: bucket_scanhist_kernel):
// a bucket is a run of consecutive micro-windows of one class -- at most ~2000 buckets in all, at least 16 k micro-windows each --
// and is counted in parts of scan_part_bins() micro-windows.  Built when the geometry (or weighted / not) changes.
static int scan_bucket_tables(gtx_ctx *c, const int32_t *classLen, int nClasses, int step, bool weighted)
{
  std::vector<long long> key = c->scanKey; key.push_back(weighted ? 1 : 0);
  if (key == c->scanBktKey) return GTX_OK;
  c->scanBktKey.clear(); c->nScanParts = 0;
  c->bktS = {}; c->scanParts.reset();
  if (!c->scanInfo) HIPCHK(c, c->scanInfo.alloc(1));
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
  if (!gtx::scan_bucket_tables_ok(nB, nClasses, total)) { c->scanBktKey = key; return GTX_OK; }   // (bktS.nB == 0: the general kernels serve)
  int rc = build_bucket_tables(c, c->bktS, k, nClasses, true); if (rc) return rc;
  if (c->bktS.nB > 0) {
    HIPCHK(c, upload(c->scanParts, parts.data(), parts.size()));
    c->nScanParts = (int)parts.size();
  }
  c->scanBktKey = key;
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
  return partition_plan(c, c->bktS, n, a.nClasses, dW != nullptr, p, w, yes);
}

// one batch of reads by the partition path: into the micro-window histogram (zeroed by the caller), or -- d_windows not null -- the
// parts write the windows themselves (gtx::launch_scan_bucketed)
static int scan_hist_bucketed(gtx_ctx *c, const void *dR, const int *dW, int64_t n, const gtx::ScanArgs &a, const gtx::BucketPlan &p, const gtx::BucketWork &w, u64 *d_windows)
{
  gtx::CountArgs ca = {};                                      // what the partition pass reads of it; its counts of dropped reads go nowhere
  ca.nClasses = a.nClasses; ca.zeroLenOk = 0; ca.coverRule = 1; ca.keyCenter = a.center; ca.info = c->scanInfo.get(); ca.indexBase = 0;
  HIPCHK(c, gtx::launch_scan_bucketed(dR, dW, n, ca, a, c->bktS.view(), w, p, c->scanParts.get(), c->nScanParts, c->stream, d_windows));
  return GTX_OK;
}

// one batch of reads into the micro-window histogram (zeroed by the caller): the partition path or the general kernel
static int scan_hist_any(gtx_ctx *c, const void *dR, const int *dW, int64_t n, const gtx::ScanArgs &a, const int32_t *classLen, bool unsorted)
{
  gtx::BucketPlan p; gtx::BucketWork w; bool part;
  int rc = scan_partition_plan(c, dW, n, a, classLen, unsorted, &p, &w, &part); if (rc) return rc;
  if (part) return scan_hist_bucketed(c, dR, dW, n, a, p, w, nullptr);
  HIPCHK(c, gtx::launch_scan_hist(dR, dW, n, a, c->stream));
  return GTX_OK;
}

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
  if (c->scanTotalWindows > 0 && !d_out) return fail(c, GTX_E_ARG, "gtx_scan: null output");
  const bool micro64 = d_weights != nullptr;
  const size_t microBytes = (size_t)c->scanTotalMicro * (micro64 ? 8 : 4);
  const int *runIf = nullptr;
  if (tile > 0 && own.totalBlocks > 0) {
    HIPCHK(c, hipMemsetAsync(c->scanFlag.get(), 0, sizeof(int), c->stream));
    if (profile) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    HIPCHK(c, gtx::launch_scan_own(d_reads, d_weights, n, a, own, (u64 *)d_out, c->stream));
    if (profile) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    runIf = c->scanFlag.get();
    if (microBytes) HIPCHK(c, gtx::launch_scan_zero(c->micro.get(), (long long)microBytes, runIf, c->stream));
    HIPCHK(c, gtx::launch_scan_hist(d_reads, d_weights, n, a, c->stream, runIf));
  } else {
    // reads in no order through the partition path: its parts write the windows themselves (no micro-window array, no window pass)
    gtx::BucketPlan p; gtx::BucketWork w; bool part;
    rc = scan_partition_plan(c, (const int *)d_weights, n, a, classLen, (flags & GTX_READS_UNSORTED) != 0, &p, &w, &part); if (rc) return rc;
    const bool fused = part && gtx::scan_fused_ok(a.comb, gtx::scan_fused_max_comb(), c->scanTotalWindows, knobs);
    if (!fused && microBytes) HIPCHK(c, hipMemsetAsync(c->micro.get(), 0, microBytes, c->stream));
    if (profile) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    if (part) { rc = scan_hist_bucketed(c, d_reads, (const int *)d_weights, n, a, p, w, fused ? (u64 *)d_out : nullptr); if (rc) return rc; }
    else HIPCHK(c, gtx::launch_scan_hist(d_reads, d_weights, n, a, c->stream));
    if (profile) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    if (fused) return GTX_OK;
  }
  HIPCHK(c, gtx::launch_scan_windows(c->micro.get(), micro64, a, c->scanTotalTiles, (u64 *)d_out, c->stream, runIf));
  return GTX_OK;
}

// a host-buffer call's reads brought into ONE device buffer (pageable memory through the page-locked slots), so that the
// owner-computes scan can be a single launch over all of them
static int stage_resident(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, void **dR, int **dW)
{
  if (c->directPending) { HIPCHK(c, hipStreamSynchronize(c->copyStream)); c->directPending = false; }
  const size_t bytes = (size_t)n * 12, nW = weights ? (size_t)n : 0;
  if (bytes > c->resReads.cap || nW > c->resWeights.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipStreamSynchronize(c->copyStream));
    HIPCHK(c, c->resReads.reserve(bytes));
    HIPCHK(c, c->resWeights.reserve(nW));
  }
  const bool direct = is_pinned(reads) && (!weights || is_pinned(weights));
  const int64_t batch = c->batchReads;
  const size_t slotBytes = (size_t)std::min<int64_t>(n, batch) * 16;
  if (!direct && (slotBytes > c->pin[0].cap || slotBytes > c->pin[1].cap)) {
    HIPCHK(c, hipStreamSynchronize(c->copyStream));
    for (int k = 0; k < 2; k++) HIPCHK(c, c->pin[k].reserve(slotBytes));
    c->slotBusy[0] = c->slotBusy[1] = false;
  }
  // the kernels of the previous call (the context's stream) may still be reading the resident buffer
  HIPCHK(c, hipEventRecord(c->evRes[0], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->copyStream, c->evRes[0], 0));
  for (int64_t off = 0; off < n; off += batch) {
    const int64_t cnt = std::min(batch, n - off);
    const char *srcR = (const char *)(reads + 3 * off), *srcW = (const char *)(weights ? weights + off : nullptr);
    int slot = -1;
    if (!direct) {
      slot = (int)(c->stageSeq++ & 1);
      if (c->slotBusy[slot]) HIPCHK(c, hipEventSynchronize(c->evCopied[slot]));      // the DMA out of this page-locked slot is done
      parallel_copy(c->pin[slot].get(), srcR, (size_t)cnt * 12, c->copyThreads);
      if (weights) parallel_copy(c->pin[slot].get() + (size_t)cnt * 12, srcW, (size_t)cnt * 4, c->copyThreads);
      srcR = c->pin[slot].get(); srcW = c->pin[slot].get() + (size_t)cnt * 12;
    }
    HIPCHK(c, hipMemcpyAsync((char *)c->resReads.get() + (size_t)off * 12, srcR, (size_t)cnt * 12, hipMemcpyHostToDevice, c->copyStream));
    if (weights) HIPCHK(c, hipMemcpyAsync(c->resWeights.get() + off, srcW, (size_t)cnt * 4, hipMemcpyHostToDevice, c->copyStream));
    if (slot >= 0) { HIPCHK(c, hipEventRecord(c->evCopied[slot], c->copyStream)); c->slotBusy[slot] = true; }
  }
  c->directPending = direct;
  HIPCHK(c, hipEventRecord(c->evRes[1], c->copyStream));                              // everything has arrived before the scan starts
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->evRes[1], 0));
  *dR = c->resReads.get(); *dW = weights ? c->resWeights.get() : nullptr;
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
  c->profThis = c->prof && (c->profEvery <= 1 || (c->profSeq++ % c->profEvery) == 0);
  if (c->profThis) c->ev = c->evRing[c->profCalls % gtx_ctx::kProfSlots];
  int rc = scan_launch(c, d_reads, d_weights, n, classLen, nClasses, step, size, prep, flags, classOff, d_out, c->profThis); if (rc) return rc;
  if (c->profThis) { if (c->profEvery <= 1) HIPCHK(c, hipEventRecord(c->ev[3], c->stream)); c->profCalls++; }
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
    if (c->scanTotalMicro > 0) HIPCHK(c, hipMemsetAsync(c->micro.get(), 0, (size_t)c->scanTotalMicro * (micro64 ? 8 : 4), c->stream));
    rc = stage_batches(c, reads, weights, n, [&](const void *dR, const int *dW, int64_t cnt, int64_t off) -> int {
      const bool unsorted = (flags & GTX_READS_UNSORTED) || host_reads_look_unsorted(reads + 3 * off, cnt);
      return scan_hist_any(c, dR, dW, cnt, a, classLen, unsorted);
    });
    if (rc) return rc;
    HIPCHK(c, gtx::launch_scan_windows(c->micro.get(), micro64, a, c->scanTotalTiles, c->out.get(), c->stream));
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
  HIPCHK(c, hipStreamSynchronize(c->copyStream));
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
  if (c->scan.open || c->streamOpen || c->covOpen) return fail(c, GTX_E_STATE, "gtx_scan_begin: a call is open");
  HIPCHK(c, hipSetDevice(c->device));
  int64_t extent = 0;
  for (int i = 0; i < nClasses; i++) extent = std::max<int64_t>(extent, classOff[i] + gtx_scan_n_windows(classLen[i] < 0 ? 0 : classLen[i], step, size));
  int rc = ensure_out(c, (size_t)extent); if (rc) return rc;
  if (extent > 0) HIPCHK(c, hipMemsetAsync(c->out.get(), 0, (size_t)extent * sizeof(u64), c->stream));
  gtx_ctx::ScanOpen &s = c->scan;
  rc = scan_prepare(c, classLen, nClasses, step, size, classOff, &s.a); if (rc) return rc;
  s.a.center = prep == 'c'; s.a.sortedRule = (flags & GTX_ZERO_LENGTH_OK) ? 1 : 0;
  s.weighted = weighted != 0; s.classLen.assign(classLen, classLen + nClasses); s.extent = extent; s.prep = prep; s.flags = flags;
  if (c->scanTotalMicro > 0) HIPCHK(c, hipMemsetAsync(c->micro.get(), 0, (size_t)c->scanTotalMicro * (s.weighted ? 8 : 4), c->stream));
  if (!s.labelSum) HIPCHK(c, s.labelSum.alloc(1));
  HIPCHK(c, hipMemsetAsync(s.labelSum.get(), 0, sizeof(unsigned long long), c->stream));
  s.open = true;
  return GTX_OK;
}

int gtx_scan_add(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, uint32_t flags)
{
  if (!c) return GTX_E_ARG;
  if (!c->scan.open) return fail(c, GTX_E_STATE, "gtx_scan_add: gtx_scan_begin has not been called");
  if (n < 0 || (n > 0 && !reads) || (c->scan.weighted && n > 0 && !weights) || (!c->scan.weighted && weights)) return fail(c, GTX_E_ARG, "gtx_scan_add: bad argument (weights as announced to gtx_scan_begin)");
  HIPCHK(c, hipSetDevice(c->device));
  gtx_ctx::ScanOpen &s = c->scan;
  return stage_batches(c, reads, weights, n, [&](const void *dR, const int *dW, int64_t cnt, int64_t off) -> int {
    const bool unsorted = (flags & GTX_READS_UNSORTED) || host_reads_look_unsorted(reads + 3 * off, cnt);
    return scan_hist_any(c, dR, dW, cnt, s.a, s.classLen.data(), unsorted);
  });
}

int gtx_scan_end(gtx_ctx *c, uint64_t *out, int64_t *labelSum)
{
  if (!c) return GTX_E_ARG;
  if (!c->scan.open) return fail(c, GTX_E_STATE, "gtx_scan_end: gtx_scan_begin has not been called");
  gtx_ctx::ScanOpen &s = c->scan;
  s.open = false;
  if (s.extent > 0 && !out) return fail(c, GTX_E_ARG, "gtx_scan_end: null output");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gtx::launch_scan_windows(c->micro.get(), s.weighted, s.a, c->scanTotalTiles, c->out.get(), c->stream));
  if (s.extent > 0) HIPCHK(c, hipMemcpyAsync(out, c->out.get(), (size_t)s.extent * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  unsigned long long sum = 0;
  HIPCHK(c, hipMemcpyAsync(&sum, s.labelSum.get(), sizeof sum, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->copyStream));
  if (labelSum) *labelSum = (int64_t)sum;
  return GTX_OK;
}

// gtx_scan_end with the windows left on the device: the sliding sums are written into the slot's own vector (zero first: class_offsets
// may leave gaps), nothing but the label sum comes to the host
int gtx_scan_end_keep(gtx_ctx *c, int slot, int64_t *labelSum)
{
  if (!c) return GTX_E_ARG;
  if (!c->scan.open) return fail(c, GTX_E_STATE, "gtx_scan_end_keep: gtx_scan_begin has not been called");
  gtx_ctx::ScanOpen &s = c->scan;
  s.open = false;                                                    // (a refused slot ends the scan too, like gtx_scan_end's null output)
  if (slot < 0 || slot >= GTX_SCAN_KEEP_SLOTS) return fail(c, GTX_E_ARG, "gtx_scan_end_keep: slot out of range");
  HIPCHK(c, hipSetDevice(c->device));
  if ((size_t)s.extent > c->kept[slot].cap || !c->kept[slot]) {
    HIPCHK(c, hipStreamSynchronize(c->stream));                      // a selection may still be reading what the slot held
    HIPCHK(c, c->kept[slot].alloc((size_t)std::max<int64_t>(s.extent, 1)));
  }
  c->keptLen[slot] = s.extent;
  if (s.extent > 0) HIPCHK(c, hipMemsetAsync(c->kept[slot].get(), 0, (size_t)s.extent * sizeof(u64), c->stream));
  HIPCHK(c, gtx::launch_scan_windows(c->micro.get(), s.weighted, s.a, c->scanTotalTiles, c->kept[slot].get(), c->stream));
  unsigned long long sum = 0;
  HIPCHK(c, hipMemcpyAsync(&sum, s.labelSum.get(), sizeof sum, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->copyStream));
  if (labelSum) *labelSum = (int64_t)sum;
  return GTX_OK;
}

int gtx_scan_kept(gtx_ctx *c, int slot, void **d_ptr, int64_t *n_windows)
{
  if (!c) return GTX_E_ARG;
  if (slot < 0 || slot >= GTX_SCAN_KEEP_SLOTS) return fail(c, GTX_E_ARG, "gtx_scan_kept: slot out of range");
  if (!c->kept[slot]) return fail(c, GTX_E_STATE, "gtx_scan_kept: the slot is empty");
  if (d_ptr) *d_ptr = c->kept[slot].get();
  if (n_windows) *n_windows = c->keptLen[slot];
  return GTX_OK;
}

int gtx_scan_drop(gtx_ctx *c, int slot)
{
  if (!c) return GTX_E_ARG;
  if (slot < -1 || slot >= GTX_SCAN_KEEP_SLOTS) return fail(c, GTX_E_ARG, "gtx_scan_drop: slot out of range");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < GTX_SCAN_KEEP_SLOTS; k++) if (slot == -1 || slot == k) { c->kept[k].reset(); c->keptLen[k] = 0; }
  return GTX_OK;
}

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
  const int64_t nt = gtx::select_tiles(n_windows);
  if (!c->selTotal) HIPCHK(c, c->selTotal.alloc(1));
  if (stride * n_tested > c->selTab.cap || (size_t)nt > c->selCount.cap || (size_t)nt + 1 > c->selBase.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->selTab.reserve(stride * n_tested)); HIPCHK(c, c->selCount.reserve((size_t)nt)); HIPCHK(c, c->selBase.reserve((size_t)nt + 1));
  }
  // (the tables are pageable host memory: these copies return when the source has been read)
  for (int f = 0; f < n_tested; f++) HIPCHK(c, hipMemcpyAsync(c->selTab.get() + f * stride, kcrit[f], stride * sizeof(int), hipMemcpyHostToDevice, c->stream));
  a.tab = c->selTab.get(); a.nTested = n_tested; a.W = W; a.n = n_windows;
  HIPCHK(c, gtx::launch_window_select(a, c->selCount.get(), c->selBase.get(), capacity, (long long *)d_ordinals, (int *)d_rows, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->selTotal.get(), c->selBase.get() + nt, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_kept = *c->selTotal.get();
  return GTX_OK;
}

int gtx_window_select(gtx_ctx *c, const void *const *d_tested, const void *const *d_control, int32_t n_tested, int64_t n_windows, int32_t W,
                      const int32_t *const *kcrit, int64_t capacity, int64_t *ordinals, int32_t *rows, int64_t *n_kept)
{
  if (!c) return GTX_E_ARG;
  if (capacity < 0 || (capacity > 0 && (!ordinals || !rows))) return fail(c, GTX_E_ARG, "gtx_window_select: null output");
  if (n_tested < 1 || n_tested > gtx::kSelectMaxTested) return fail(c, GTX_E_ARG, "gtx_window_select: 1 to 4 tested vectors, their tables and n_kept are required");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t cols = (size_t)n_tested * ((d_control && d_control[0]) ? 2 : 1);
  if ((size_t)capacity > c->selOrd.cap || (size_t)capacity * cols > c->selRows.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->selOrd.reserve((size_t)capacity)); HIPCHK(c, c->selRows.reserve((size_t)capacity * cols));
  }
  int rc = gtx_window_select_device(c, d_tested, d_control, n_tested, n_windows, W, kcrit, capacity, c->selOrd.get(), c->selRows.get(), n_kept); if (rc) return rc;
  const size_t got = (size_t)std::min<int64_t>(*n_kept, capacity);
  if (got) {
    HIPCHK(c, hipMemcpy(ordinals, c->selOrd.get(), got * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(rows, c->selRows.get(), got * cols * sizeof(int), hipMemcpyDeviceToHost));
  }
  return GTX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// region text tokenised on the device (gtx_text.hip)
// ---------------------------------------------------------------------------------------------
enum TextMode { TEXT_COUNT, TEXT_COVER, TEXT_SCAN };

// A block of text into the slot whose turn it is, and tokenised there (launch_tokenize enqueued on the context's stream): the front
// of add_text and gtx_subset_text.  grouped: the strand-aware outputs (tri2 / w2) are made too when the rules are strand-aware.
// *tp = the slot, *ticket its number; *empty: a block without lines -- nothing was enqueued but the slot's evParsed, its verdict is 0.
static int text_stage(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, bool grouped, int scanRules,
                      unsigned long long *labelSum, bool sam, TextSlot **tp, int *ticket, bool *empty)
{
  HIPCHK(c, hipSetDevice(c->device));
  const int slot = (int)(c->textSeq & 1);
  TextSlot &t = c->text[slot];
  *ticket = slot; *tp = &t; *empty = false;
  if (!t.evParsed) {
    HIPCHK(c, hipEventCreateWithFlags(&t.evParsed, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&t.evConsumed, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&t.evCopied, hipEventDisableTiming));
    HIPCHK(c, t.flag.alloc(1)); HIPCHK(c, t.hostFlag.alloc(1)); HIPCHK(c, t.seam.alloc(4096));
    HIPCHK(c, t.sum.alloc(1)); HIPCHK(c, hipMemset(t.sum.get(), 0, sizeof(unsigned long long)));
  }
  if (t.busy) { HIPCHK(c, hipEventSynchronize(t.evConsumed)); t.busy = false; }          // the block before last has been counted: its buffers are free
  c->textSeq++;
  if (nLines == 0 || bytes == 0) { *t.hostFlag.get() = 0; HIPCHK(c, hipEventRecord(t.evParsed, c->stream)); *empty = true; return GTX_OK; }
  const size_t nSeg = (bytes + 1023) / 1024;
  if (bytes + 128 > t.text.cap) HIPCHK(c, t.text.alloc(bytes + (bytes >> 3) + 4096));              // (128 bytes beyond the block kept free)
  if (nSeg + 4 > t.seg.cap) HIPCHK(c, t.seg.alloc(nSeg + (nSeg >> 3) + 16));
  if ((size_t)nLines > t.w.cap) {
    t.nl.reset(); t.tri.reset(); t.w.reset();
    const size_t cap = (size_t)nLines + ((size_t)nLines >> 3) + 1024;
    HIPCHK(c, t.nl.alloc(cap)); HIPCHK(c, t.tri.alloc(3 * cap)); HIPCHK(c, t.w.alloc(cap));
  }
  // the names' tables: per set of names (rebuilt when they change)
  {
    std::string blob; std::vector<int32_t> table; unsigned mask = 0;
    size_t total = 0; for (int i = 0; i < r->n_chrom; i++) total += strlen(r->chrom_names[i]) + 1;
    std::string key; key.reserve(total);
    for (int i = 0; i < r->n_chrom; i++) { key += r->chrom_names[i]; key += '\n'; }
    if (key != c->textBlob || !c->textNames) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      gtxtext::build_tables(*r, &table, &mask, &blob);
      c->textTable.reset(); c->textNames.reset();
      HIPCHK(c, c->textTable.alloc(table.size()));
      HIPCHK(c, c->textNames.alloc(blob.size() + 4096 * 2 + 16));
      HIPCHK(c, hipMemcpy(c->textTable.get(), table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice));
      if (!blob.empty()) HIPCHK(c, hipMemcpy(c->textNames.get(), blob.data(), blob.size(), hipMemcpyHostToDevice));
      c->textMask = mask; c->textBlobLen = (unsigned)blob.size(); c->textBlob = key;
    }
  }
  gtxtext::TextTables tabs; tabs.table = c->textTable.get(); tabs.tableMask = c->textMask; tabs.names = c->textNames.get(); tabs.prevOff = 0; tabs.prevLen = 0;
  if (r->have_prev && r->prev_chrom) {
    const size_t len = strlen(r->prev_chrom);
    if (len > 0 && len < 4096) {                                       // the seam's name behind the names, one place per slot
      memcpy(t.seam.get(), r->prev_chrom, len);
      tabs.prevOff = c->textBlobLen + (unsigned)slot * 4096; tabs.prevLen = (unsigned)len;
      HIPCHK(c, hipMemcpyAsync(c->textNames.get() + tabs.prevOff, t.seam.get(), len, hipMemcpyHostToDevice, c->stream));
    }
  }
  // the text: page-locked memory is read where it is, anything else goes through a page-locked slot of the context
  const char *src = text;
  if (!is_pinned(text)) {
    if (bytes > t.pin.cap) HIPCHK(c, t.pin.alloc(bytes + (bytes >> 3)));
    parallel_copy(t.pin.get(), text, bytes, c->copyThreads);
    src = t.pin.get();
  }
  HIPCHK(c, hipMemcpyAsync(t.text.get(), src, bytes, hipMemcpyHostToDevice, c->copyStream));
  HIPCHK(c, hipEventRecord(t.evCopied, c->copyStream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, t.evCopied, 0));
  HIPCHK(c, hipMemsetAsync(t.flag.get(), 0, sizeof(int), c->stream));
  grouped = grouped && r->strand_aware;
  if (grouped && (size_t)nLines > t.w2.cap) {
    t.tri2.reset(); t.blk.reset(); t.w2.reset();
    HIPCHK(c, t.tri2.alloc(3 * t.w.cap)); HIPCHK(c, t.blk.alloc(t.w.cap / 128 + 4)); HIPCHK(c, t.w2.alloc(t.w.cap));
  }
  gtxtext::TextDevice d; d.text = t.text.get(); d.segCount = t.seg.get(); d.nl = t.nl.get(); d.tri = t.tri.get(); d.w = t.w.get(); d.flag = t.flag.get();
  d.tri2 = grouped ? t.tri2.get() : nullptr; d.w2 = grouped ? t.w2.get() : nullptr; d.blkMinus = grouped ? t.blk.get() : nullptr;
  d.labelSum = labelSum; d.blockSum = t.sum.get();
  HIPCHK(c, gtxtext::launch_tokenize(d, tabs, *r, bytes, (unsigned)nLines, c->stream, scanRules, sam));
  return GTX_OK;
}

static int add_text(gtx_ctx *c, TextMode mode, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, uint32_t flags, int *ticket)
{
  const bool coverage = mode == TEXT_COVER;
  const char *who = mode == TEXT_SCAN ? "gtx_scan_add_text" : coverage ? "gtx_coverage_add_text" : "gtx_count_add_text";
  if (mode == TEXT_SCAN ? !c->scan.open : coverage ? !c->covOpen : !c->streamOpen) return fail(c, GTX_E_STATE, "gtx_*_add_text: no open count / coverage / scan call");
  if (mode == TEXT_SCAN && r && (r->max_label_value > 1) != c->scan.weighted) return fail(c, GTX_E_ARG, "gtx_scan_add_text: the rules' label weights do not match gtx_scan_begin's");
  if (!text || !r || !ticket || nLines < 0 || bytes >= (1ull << 32) - 4096 || nLines >= (1ll << 31) || r->n_chrom < 0 || (r->n_chrom > 0 && !r->chrom_names))
    { c->err = std::string(who) + ": bad argument"; return GTX_E_ARG; }
  const bool sam = (flags & GTX_TEXT_SAM) != 0;                  // (the format of the text, not a flag of the count)
  flags &= ~GTX_TEXT_SAM;
  TextSlot *tp = nullptr; bool empty = false;
  {
    int rc = text_stage(c, text, bytes, nLines, r, true, mode == TEXT_SCAN ? (c->scan.a.sortedRule ? 2 : 1) : 0,
                        mode == TEXT_SCAN ? c->scan.labelSum.get() : nullptr, sam, &tp, ticket, &empty);
    if (rc || empty) return rc;
  }
  TextSlot &t = *tp;
  const int *triOut = r->strand_aware ? t.tri2.get() : t.tri.get();
  HIPCHK(c, hipMemcpyAsync(t.hostFlag.get(), t.flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(t.evParsed, c->stream));
  // ... and counted where the triples are
  const int *dW = r->max_label_value > 1 ? (r->strand_aware ? t.w2.get() : t.w.get()) : nullptr;
  const int64_t seen = c->streamSeen;
  int rc = GTX_OK;
  if (mode == TEXT_SCAN) {
    // (a block of a sorted stream is in order: the general kernels aggregate runs of equal micro-windows; any other block: the partition path)
    rc = scan_hist_any(c, triOut, dW, nLines, c->scan.a, c->scan.classLen.data(), (flags & GTX_READS_UNSORTED) != 0); if (rc) return rc;
    HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
    t.busy = true;
    return GTX_OK;
  }
  if (coverage) {
    if (flags & GTX_GAPS_FORMULA) { rc = merge_prepare(c, flags, 2); if (rc) return rc; }
    rc = cover_launch(c, triOut, dW, nLines, seen, flags, (flags & GTX_READS_UNSORTED) != 0 || !(flags & GTX_READS_SORTED)); if (rc) return rc;
  } else {
    rc = merge_prepare(c, flags, 0); if (rc) return rc;
    const bool streaming = (flags & (GTX_READS_SORTED | GTX_CHECK_SORTED)) != 0;
    if (!streaming) c->tileSumsValid = false;
    if (streaming) HIPCHK(c, gtx::launch_count(triOut, dW, nLines, count_args(c, c->ix.hist, flags & ~GTX_CHECK_SORTED, nLines, seen), true, c->stream));
    else { rc = launch_unsorted(c, triOut, dW, nLines, count_args(c, c->ix.hist, flags, nLines, seen)); if (rc) return rc; }
    rc = pairs_batch(c, triOut, dW, nLines); if (rc) return rc;
  }
  rc = merge_batch(c, triOut, dW, nLines); if (rc) return rc;
  HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
  t.busy = true;
  c->streamSeen += nLines;
  return GTX_OK;
}

extern "C" {
int gtx_count_add_text(gtx_ctx *c, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket)
{ return c ? add_text(c, TEXT_COUNT, text, bytes, n_lines, rules, flags, ticket) : GTX_E_ARG; }
int gtx_coverage_add_text(gtx_ctx *c, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket)
{ return c ? add_text(c, TEXT_COVER, text, bytes, n_lines, rules, flags, ticket) : GTX_E_ARG; }
int gtx_scan_add_text(gtx_ctx *c, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket)
{ return c ? add_text(c, TEXT_SCAN, text, bytes, n_lines, rules, flags, ticket) : GTX_E_ARG; }
int gtx_text_result(gtx_ctx *c, int ticket, int *needs_host)
{
  if (!c || !needs_host || (ticket & ~1)) return c ? fail(c, GTX_E_ARG, "gtx_text_result: bad argument") : GTX_E_ARG;
  TextSlot &t = c->text[ticket];
  if (!t.evParsed) return fail(c, GTX_E_STATE, "gtx_text_result: no such block");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(t.evParsed));
  *needs_host = *t.hostFlag.get();
  return GTX_OK;
}

// text -> triples in line order -> hits -> verbatim check -> select, scan, gather; everything enqueued, the verdict and the totals
// on their way to the host behind it
int gtx_subset_text(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, uint32_t flags, int *ticket)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_subset_text: gtx_set_refs has not been called");
  if (!text || !r || !ticket || nLines < 0 || bytes >= (1ull << 32) - 4096 || nLines >= (1ll << 31) || r->n_chrom < 0 || (r->n_chrom > 0 && !r->chrom_names) ||
      (flags & GTX_TEXT_SAM) || r->max_label_value > 1)
    return fail(c, GTX_E_ARG, "gtx_subset_text: bad argument");
  if (c->text[c->textSeq & 1].subsetPending) return fail(c, GTX_E_STATE, "gtx_subset_text: the result of the block before last has not been fetched (gtx_subset_result)");
  const int mode = join_mode(c, flags);
  { int rc = join_prepare(c); if (rc) return rc; }
  TextSlot *tp = nullptr; bool empty = false;
  { int rc = text_stage(c, text, bytes, nLines, r, false, 0, nullptr, false, &tp, ticket, &empty); if (rc) return rc; }
  TextSlot &t = *tp;
  if (!t.hostTotal) HIPCHK(c, t.hostTotal.alloc(2));
  t.hostTotal.get()[0] = t.hostTotal.get()[1] = 0;
  t.subsetPending = true;
  if (empty) return GTX_OK;
  const size_t nTiles = gtxtext::subset_tiles((unsigned)nLines);
  if ((size_t)nLines > t.hits.cap) HIPCHK(c, t.hits.alloc(t.w.cap));
  if (2 * (nTiles + 1) > t.tile.cap) HIPCHK(c, t.tile.alloc(2 * (nTiles + 1) + (nTiles >> 2)));
  if (bytes > t.out.cap) HIPCHK(c, t.out.alloc(t.text.cap));
  const gtx::JoinQueries q{t.tri.get(), nullptr, nullptr, nLines};
  if (!c->joinInfo) HIPCHK(c, c->joinInfo.alloc(1));
  if ((size_t)nLines > c->joinOff.cap) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, c->joinOff.grow((size_t)nLines)); }   // (the block before may still be narrowing out of it)
  HIPCHK(c, gtx::launch_join_count(q, c->rx.pairAll.ix, ref_blocks(c), mode & ~gtx::JOIN_CHECK, c->joinOff.get(), c->joinInfo.get(), c->stream));
  HIPCHK(c, gtx::launch_query_narrow(c->joinOff.get(), nLines, t.hits.get(), c->stream));
  HIPCHK(c, gtxtext::launch_verbatim(t.text.get(), t.nl.get(), (unsigned)nLines, t.flag.get(), c->stream));
  const gtxtext::SubsetDevice d{t.text.get(), t.nl.get(), (unsigned)nLines, t.hits.get(), (flags & GTX_SUBSET_INVERT) ? 1 : 0, t.flag.get(), t.tile.get(), t.out.get()};
  HIPCHK(c, gtxtext::launch_subset_gather(d, c->stream));
  HIPCHK(c, hipMemcpyAsync(t.hostFlag.get(), t.flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&t.hostTotal.get()[0], t.tile.get() + nTiles, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&t.hostTotal.get()[1], t.tile.get() + 2 * nTiles + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(t.evParsed, c->stream));
  HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
  t.busy = true;
  return GTX_OK;
}

int gtx_subset_result(gtx_ctx *c, int ticket, int *needs_host, char *out, size_t *out_bytes, int64_t *n_selected)
{
  if (!c || !needs_host || !out_bytes || (ticket & ~1)) return c ? fail(c, GTX_E_ARG, "gtx_subset_result: bad argument") : GTX_E_ARG;
  TextSlot &t = c->text[ticket];
  if (!t.evParsed || !t.subsetPending) return fail(c, GTX_E_STATE, "gtx_subset_result: no such block");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(t.evParsed));
  t.subsetPending = false;
  *needs_host = *t.hostFlag.get();
  *out_bytes = 0;
  if (n_selected) *n_selected = 0;
  if (*needs_host) return GTX_OK;
  const size_t n = (size_t)t.hostTotal.get()[0];
  if (n > 0 && !out) return fail(c, GTX_E_ARG, "gtx_subset_result: bad argument");
  // (on the copy stream: the context's own may already hold the kernels of the block after this one)
  if (n > 0) { HIPCHK(c, hipMemcpyAsync(out, t.out.get(), n, hipMemcpyDeviceToHost, c->copyStream)); HIPCHK(c, hipStreamSynchronize(c->copyStream)); }
  *out_bytes = n;
  if (n_selected) *n_selected = (int64_t)t.hostTotal.get()[1];
  return GTX_OK;
}
}

extern "C" {

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
  c->profThis = c->prof && (c->profEvery <= 1 || (c->profSeq++ % c->profEvery) == 0);
  if (c->profThis) { c->ev = c->evRing[c->profCalls % gtx_ctx::kProfSlots]; HIPCHK(c, hipEventRecord(c->ev[1], c->stream)); }
  const bool streaming = (flags & (GTX_READS_SORTED | GTX_CHECK_SORTED)) != 0;
  if (!streaming) c->tileSumsValid = false;
  if (n > 0) {
    if (streaming) HIPCHK(c, gtx::launch_count(d_reads, d_weights, n, count_args(c, c->ix.hist, flags, n, 0, COUNT_SHARE), true, c->stream));
    else { rc = launch_unsorted(c, d_reads, d_weights, n, count_args(c, c->ix.hist, flags, n, 0, COUNT_SHARE)); if (rc) return rc; }
  }
  if (c->profThis) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  u64 *dst = direct_out ? (u64 *)direct_out : c->out.get() + (size_t)(slot % GTXI_SHARE_SLOTS) * c->nRefs + c->share.offset;
  rc = count_end(c, dst, true, direct_out != nullptr); if (rc) return rc;
  if (c->profThis) { if (c->profEvery <= 1) HIPCHK(c, hipEventRecord(c->ev[3], c->stream)); c->profCalls++; }
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
  c->profThis = c->prof && (c->profEvery <= 1 || (c->profSeq++ % c->profEvery) == 0);
  if (c->profThis) { c->ev = c->evRing[c->profCalls % gtx_ctx::kProfSlots]; HIPCHK(c, hipEventRecord(c->ev[1], run)); }
  const bool keepDefault = c->tileSumsValid;
  c->tileSumsValid = true;
  gtx::CountArgs a = count_args(c, h, flags, n, 0, COUNT_SHARE_ASYNC, d_weights == nullptr);   // (clears c->tileSumsValid when the kernel leaves the tile sums to the finalize step)
  a.info = info;
  const bool sumsValid = c->tileSumsValid;
  c->tileSumsValid = keepDefault;
  if (n > 0) HIPCHK(c, gtx::launch_count(d_reads, d_weights, n, a, true, run));
  if (c->profThis) HIPCHK(c, hipEventRecord(c->ev[2], run));
  // direct_out (may be null): the caller's result vector in file order (n_refs entries) -- the member's regions go to their places in it
  u64 *dst = direct_out ? (u64 *)direct_out : c->out.get() + (size_t)(slot % GTXI_SHARE_SLOTS) * c->nRefs + c->share.offset;
  const gtx::FinalizeShare fs = {c->share.tiles.get(), c->share.nTiles, c->share.regions.get(), c->share.nRegions, direct_out != nullptr};
  int rc = finalize_set(c, h, sumsValid, dst, info, infoNext, run, &fs, a.hist32 != 0 && n > 0); if (rc) return rc;
  if (c->profThis) { if (c->profEvery <= 1) HIPCHK(c, hipEventRecord(c->ev[3], run)); c->profCalls++; }
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
  if (c->directPending) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->copyStream)); c->directPending = false; }
  return GTX_OK;
}

hipStream_t gtxi_stream(gtx_ctx *c) { return c->stream; }
int gtxi_device(gtx_ctx *c) { return c->device; }
void gtxi_set_error(gtx_ctx *c, const char *msg) { c->err = msg; }

// ---------------------------------------------------------------------------------------------
// link (kernels: gtx_link.hip)
// ---------------------------------------------------------------------------------------------
static int link_mode(uint32_t flags, bool haveValues, int *mode)
{
  const uint32_t f = flags & (GTX_LINK_SUM | GTX_LINK_MIN | GTX_LINK_MAX);
  if (flags & ~(GTX_LINK_SUM | GTX_LINK_MIN | GTX_LINK_MAX)) return GTX_E_ARG;
  if (f & (f - 1)) return GTX_E_ARG;                                 // at most one fold
  if (f && !haveValues) return GTX_E_ARG;
  *mode = f == GTX_LINK_SUM ? gtx::LINK_SUM : f == GTX_LINK_MIN ? gtx::LINK_MIN : f == GTX_LINK_MAX ? gtx::LINK_MAX : gtx::LINK_NONE;
  return GTX_OK;
}

// the info block of a gtx_link_device call that has not been synchronised yet goes to its caller's struct before the page-locked
// block is used again
static int link_settle(gtx_ctx *c)
{
  if (!c->linkPending) return GTX_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const gtx::LinkInfo &h = c->linkHost.get()[0];
  c->linkPending->n_groups = h.nGroups; c->linkPending->first_unsorted = h.firstUnsortedOut;
  c->linkPending = nullptr;
  return GTX_OK;
}

// the kernels and the copy of the info block into page-locked memory, enqueued
static int link_enqueue(gtx_ctx *c, const void *d_tri, const void *d_vals, int64_t n, int64_t d, int mode, void *d_head, void *d_cnt, void *d_stop, void *d_val)
{
  const size_t nt = (size_t)gtx::link_tiles(n);
  HIPCHK(c, c->linkAgg.reserve(nt)); HIPCHK(c, c->linkPrefix.reserve(nt)); HIPCHK(c, c->linkBits.reserve(nt * (gtx::kLinkTile / 64) + 1));
  HIPCHK(c, c->linkHeads.reserve(nt)); HIPCHK(c, c->linkBase.reserve(nt + 1));
  if (!c->linkInfo) HIPCHK(c, c->linkInfo.alloc(1));
  if (!c->linkHost) HIPCHK(c, c->linkHost.alloc(1));
  gtx::LinkWork w;
  w.tileAgg = c->linkAgg.get(); w.tilePrefix = c->linkPrefix.get(); w.bits = c->linkBits.get(); w.tileHeads = c->linkHeads.get();
  w.tileHeadBase = c->linkBase.get(); w.info = c->linkInfo.get();
  HIPCHK(c, gtx::launch_link((const int *)d_tri, (const long long *)d_vals, n, d, mode, w, (unsigned *)d_head, (unsigned *)d_cnt, (int *)d_stop,
                             (long long *)d_val, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->linkHost.get(), c->linkInfo.get(), sizeof(gtx::LinkInfo), hipMemcpyDeviceToHost, c->stream));
  return GTX_OK;
}

int gtx_link_device(gtx_ctx *c, const void *d_triples, const void *d_values, int64_t n, int64_t max_difference, uint32_t flags,
                    void *d_head, void *d_count, void *d_stop, void *d_value, gtx_link_info *info)
{
  if (!c) return GTX_E_ARG;
  int mode = 0;
  if (link_mode(flags, d_values != nullptr && d_value != nullptr, &mode)) return fail(c, GTX_E_ARG, "gtx_link_device: at most one of GTX_LINK_SUM / _MIN / _MAX, and values with it");
  if (n < 0 || n >= (1ll << 32) || !info || (n > 0 && (!d_triples || !d_head || !d_count || !d_stop))) return fail(c, GTX_E_ARG, "gtx_link_device: bad argument (n < 2^32)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = link_settle(c); if (rc) return rc; }
  info->n_groups = 0; info->first_unsorted = -1;
  if (n == 0) return GTX_OK;
  if (int rc = link_enqueue(c, d_triples, d_values, n, max_difference, mode, d_head, d_count, d_stop, d_value)) return rc;
  c->linkPending = info;
  return GTX_OK;
}

int gtx_link(gtx_ctx *c, const int32_t *triples, const int64_t *values, int64_t n, int64_t max_difference, uint32_t flags,
             uint32_t *head_out, uint32_t *count_out, int32_t *stop_out, int64_t *value_out, gtx_link_info *info)
{
  if (!c) return GTX_E_ARG;
  int mode = 0;
  if (link_mode(flags, values != nullptr && value_out != nullptr, &mode)) return fail(c, GTX_E_ARG, "gtx_link: at most one of GTX_LINK_SUM / _MIN / _MAX, and values with it");
  if (n < 0 || n >= (1ll << 32) || !info || (n > 0 && (!triples || !head_out || !count_out || !stop_out))) return fail(c, GTX_E_ARG, "gtx_link: bad argument (n < 2^32)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = link_settle(c); if (rc) return rc; }
  info->n_groups = 0; info->first_unsorted = -1;
  if (n == 0) return GTX_OK;
  const size_t m = (size_t)n;
  HIPCHK(c, c->linkTri.reserve(3 * m)); HIPCHK(c, c->linkHead.reserve(m)); HIPCHK(c, c->linkCnt.reserve(m)); HIPCHK(c, c->linkStop.reserve(m));
  if (mode) { HIPCHK(c, c->linkVals.reserve(m)); HIPCHK(c, c->linkVal.reserve(m)); }
  HIPCHK(c, hipMemcpyAsync(c->linkTri.get(), triples, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, c->stream));
  if (mode) HIPCHK(c, hipMemcpyAsync(c->linkVals.get(), values, sizeof(int64_t) * m, hipMemcpyHostToDevice, c->stream));
  if (int rc = link_enqueue(c, c->linkTri.get(), mode ? c->linkVals.get() : nullptr, n, max_difference, mode, c->linkHead.get(), c->linkCnt.get(),
                            c->linkStop.get(), mode ? c->linkVal.get() : nullptr)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const gtx::LinkInfo &h = c->linkHost.get()[0];
  info->n_groups = h.nGroups; info->first_unsorted = h.firstUnsortedOut;
  const size_t g = (size_t)h.nGroups;
  if (g) {
    HIPCHK(c, hipMemcpyAsync(head_out, c->linkHead.get(), sizeof(uint32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(count_out, c->linkCnt.get(), sizeof(uint32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(stop_out, c->linkStop.get(), sizeof(int32_t) * g, hipMemcpyDeviceToHost, c->stream));
    if (mode) HIPCHK(c, hipMemcpyAsync(value_out, c->linkVal.get(), sizeof(int64_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GTX_OK;
}

// link fed as a stream of text blocks (the tool's path): see include/gtx.h
int gtx_link_text_begin(gtx_ctx *c, int32_t n_chrom, int sorted_by_strand, int64_t capacity)
{
  if (!c) return GTX_E_ARG;
  if (n_chrom < 0 || capacity < 0 || capacity >= (1ll << 32)) return fail(c, GTX_E_ARG, "gtx_link_text_begin: bad argument (capacity < 2^32)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = link_settle(c); if (rc) return rc; }
  HIPCHK(c, c->linkTextTri.reserve(3 * (size_t)std::max<int64_t>(capacity, 1))); HIPCHK(c, c->linkMinus.reserve((size_t)std::max<int64_t>(capacity, 1)));
  c->linkTextOpen = true; c->linkTextN = 0; c->linkTextCap = capacity; c->linkTextChrom = n_chrom; c->linkTextByStrand = sorted_by_strand != 0;
  return GTX_OK;
}

int gtx_link_add_text(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, int *needs_host)
{
  if (!c) return GTX_E_ARG;
  if (!c->linkTextOpen) return fail(c, GTX_E_STATE, "gtx_link_add_text: gtx_link_text_begin has not been called");
  if (!text || !r || !needs_host || nLines < 0 || bytes >= (1ull << 32) - 4096 || nLines >= (1ll << 31) || r->n_chrom != c->linkTextChrom || (r->n_chrom > 0 && !r->chrom_names) ||
      !r->strand_aware || r->sorted_rules || r->max_label_value > 1 || c->linkTextN + nLines > c->linkTextCap)
    return fail(c, GTX_E_ARG, "gtx_link_add_text: bad argument (strand-aware rules without order or label rules, the names of gtx_link_text_begin, room for the lines)");
  *needs_host = 0;
  TextSlot *tp = nullptr; bool empty = false; int ticket = 0;
  // (the sorted scanner's rules: nothing about the interval is checked -- zero-length and inverted regions are link's to take)
  { int rc = text_stage(c, text, bytes, nLines, r, false, 2, nullptr, false, &tp, &ticket, &empty); if (rc || empty) return rc; }
  TextSlot &t = *tp;
  HIPCHK(c, gtx::launch_link_append(t.tri.get(), nLines, c->linkTextChrom, c->linkTextByStrand, c->linkTextTri.get() + 3 * c->linkTextN,
                                    c->linkMinus.get() + c->linkTextN, t.flag.get(), c->stream));
  HIPCHK(c, hipMemcpyAsync(t.hostFlag.get(), t.flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(t.evParsed, c->stream));
  HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
  t.busy = true;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (*t.hostFlag.get()) { *needs_host = 1; return GTX_OK; }           // (what was appended lies behind the end and is written over)
  c->linkTextN += nLines;
  return GTX_OK;
}

int gtx_link_add(gtx_ctx *c, const int32_t *triples, const uint8_t *minus, int64_t n)
{
  if (!c) return GTX_E_ARG;
  if (!c->linkTextOpen) return fail(c, GTX_E_STATE, "gtx_link_add: gtx_link_text_begin has not been called");
  if (n < 0 || (n > 0 && (!triples || !minus)) || c->linkTextN + n > c->linkTextCap) return fail(c, GTX_E_ARG, "gtx_link_add: bad argument");
  if (n == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->linkTextTri.get() + 3 * c->linkTextN, triples, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->linkMinus.get() + c->linkTextN, minus, (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->linkTextN += n;
  return GTX_OK;
}

int gtx_link_text_end(gtx_ctx *c, int64_t max_difference, uint32_t *head_out, int32_t *stop_out, int32_t *head_key_out, gtx_link_info *info)
{
  if (!c) return GTX_E_ARG;
  if (!c->linkTextOpen) return fail(c, GTX_E_STATE, "gtx_link_text_end: gtx_link_text_begin has not been called");
  c->linkTextOpen = false;
  const int64_t n = c->linkTextN;
  if (!info || (n > 0 && (!head_out || !stop_out || !head_key_out))) return fail(c, GTX_E_ARG, "gtx_link_text_end: bad argument");
  info->n_groups = 0; info->first_unsorted = -1;
  if (n == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t m = (size_t)n;
  HIPCHK(c, c->linkHead.reserve(m)); HIPCHK(c, c->linkCnt.reserve(m)); HIPCHK(c, c->linkStop.reserve(m)); HIPCHK(c, c->linkHeadKey.reserve(m));
  if (int rc = link_enqueue(c, c->linkTextTri.get(), nullptr, n, max_difference, gtx::LINK_NONE, c->linkHead.get(), c->linkCnt.get(), c->linkStop.get(), nullptr)) return rc;
  HIPCHK(c, gtx::launch_link_head_keys(c->linkTextTri.get(), c->linkMinus.get(), c->linkHead.get(), c->linkInfo.get(), n, c->linkTextByStrand, c->linkHeadKey.get(), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const gtx::LinkInfo &h = c->linkHost.get()[0];
  info->n_groups = h.nGroups; info->first_unsorted = h.firstUnsortedOut;
  const size_t g = (size_t)h.nGroups;
  if (g) {
    HIPCHK(c, hipMemcpyAsync(head_out, c->linkHead.get(), sizeof(uint32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(stop_out, c->linkStop.get(), sizeof(int32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(head_key_out, c->linkHeadKey.get(), sizeof(int2) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GTX_OK;
}

// ---------------------------------------------------------------------------------------------
// the neighbour passes (kernels: gtx_adjacent.hip)
// ---------------------------------------------------------------------------------------------
// the info blocks of device calls that have completed go to their callers' structs
static void adjacent_hand_over(gtx_ctx *c)
{
  if (c->adjPending) {
    const gtx::AdjInfo &h = c->adjHost.get()[0];
    c->adjPending->first_unsorted = h.firstUnsortedOut; c->adjPending->n_inclusions = h.nInclusions; c->adjPending->n_overlaps = h.nOverlaps;
    c->adjPending = nullptr;
  }
  if (c->gapPending) {
    const gtx::GapInfo &h = c->gapHost.get()[0];
    c->gapPending->n_gaps = h.nGaps; c->gapPending->first_bad = h.firstBadOut; c->gapPending->bad_kind = h.badKind;
    c->gapPending = nullptr;
  }
}

// ... before a page-locked block is used again
static int adjacent_settle(gtx_ctx *c)
{
  if (!c->adjPending && !c->gapPending) return GTX_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  adjacent_hand_over(c);
  return GTX_OK;
}

static int adjacent_enqueue(gtx_ctx *c, const void *d_tri, const void *d_minus, int64_t n, int op1, int op2, void *d_dist)
{
  HIPCHK(c, c->adjSums.reserve((size_t)gtx::adjacent_tiles(n)));
  if (!c->adjInfo) HIPCHK(c, c->adjInfo.alloc(1));
  if (!c->adjHost) HIPCHK(c, c->adjHost.alloc(1));
  HIPCHK(c, gtx::launch_adjacent((const int *)d_tri, (const unsigned char *)d_minus, n, op1, op2, (long long *)d_dist, c->adjSums.get(), c->adjInfo.get(), c->stream));
  HIPCHK(c, hipMemcpyAsync(c->adjHost.get(), c->adjInfo.get(), sizeof(gtx::AdjInfo), hipMemcpyDeviceToHost, c->stream));
  return GTX_OK;
}

static bool adjacent_args_ok(int64_t n, int op1, int op2, const void *tri, const void *info)
{
  return n >= 0 && n < (1ll << 32) && op1 >= GTX_POINT_START && op1 <= GTX_POINT_3P && op2 >= GTX_POINT_START && op2 <= GTX_POINT_3P && info && (n == 0 || tri);
}

int gtx_adjacent_device(gtx_ctx *c, const void *d_triples, const void *d_minus, int64_t n, int op1, int op2, void *d_dist, gtx_adjacent_info *info)
{
  if (!c) return GTX_E_ARG;
  if (!adjacent_args_ok(n, op1, op2, d_triples, info)) return fail(c, GTX_E_ARG, "gtx_adjacent_device: bad argument (n < 2^32, points 0..3)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = adjacent_settle(c); if (rc) return rc; }
  info->first_unsorted = -1; info->n_inclusions = 0; info->n_overlaps = 0;
  if (n == 0) return GTX_OK;
  if (int rc = adjacent_enqueue(c, d_triples, d_minus, n, op1, op2, d_dist)) return rc;
  c->adjPending = info;
  return GTX_OK;
}

int gtx_adjacent(gtx_ctx *c, const int32_t *triples, const uint8_t *minus, int64_t n, int op1, int op2, int64_t *dist_out, gtx_adjacent_info *info)
{
  if (!c) return GTX_E_ARG;
  if (!adjacent_args_ok(n, op1, op2, triples, info)) return fail(c, GTX_E_ARG, "gtx_adjacent: bad argument (n < 2^32, points 0..3)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = adjacent_settle(c); if (rc) return rc; }
  info->first_unsorted = -1; info->n_inclusions = 0; info->n_overlaps = 0;
  if (n == 0) return GTX_OK;
  const size_t m = (size_t)n;
  const bool strands = minus != nullptr && dist_out != nullptr;
  HIPCHK(c, c->adjTri.reserve(3 * m));
  if (strands) HIPCHK(c, c->adjMinus.reserve(m));
  if (dist_out) HIPCHK(c, c->adjDist.reserve(m));
  HIPCHK(c, hipMemcpyAsync(c->adjTri.get(), triples, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, c->stream));
  if (strands) HIPCHK(c, hipMemcpyAsync(c->adjMinus.get(), minus, m, hipMemcpyHostToDevice, c->stream));
  if (int rc = adjacent_enqueue(c, c->adjTri.get(), strands ? c->adjMinus.get() : nullptr, n, op1, op2, dist_out ? c->adjDist.get() : nullptr)) return rc;
  if (dist_out) HIPCHK(c, hipMemcpyAsync(dist_out, c->adjDist.get(), sizeof(int64_t) * m, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const gtx::AdjInfo &h = c->adjHost.get()[0];
  info->first_unsorted = h.firstUnsortedOut; info->n_inclusions = h.nInclusions; info->n_overlaps = h.nOverlaps;
  return GTX_OK;
}

// the arguments of both gap entries; the bounds go to the device here (they are host memory in both)
static int gaps_prepare(gtx_ctx *c, const char *who, const void *tri, int64_t n, const int64_t *bounds, int32_t n_bounds, int64_t capacity, const void *owner,
                        const void *start, const void *stop, gtx_gaps_info *info)
{
  if (n < 0 || n >= (1ll << 32) || n_bounds < 0 || (n_bounds > 0 && !bounds) || capacity < 0 || !info || (n > 0 && !tri) || (capacity > 0 && (!owner || !start || !stop)))
    return fail(c, GTX_E_ARG, (std::string(who) + ": bad argument (n < 2^32)").c_str());
  for (int32_t k = 0; k < n_bounds; k++)
    if (bounds[k] > (int64_t)INT32_MAX - 2) return fail(c, GTX_E_RANGE, (std::string(who) + ": a bound above 2^31 - 3").c_str());
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = adjacent_settle(c); if (rc) return rc; }
  info->n_gaps = 0; info->first_bad = -1; info->bad_kind = 0;
  if (n == 0) return GTX_OK;
  HIPCHK(c, c->gapBounds.reserve((size_t)std::max<int32_t>(n_bounds, 1)));
  if (n_bounds > 0) HIPCHK(c, hipMemcpyAsync(c->gapBounds.get(), bounds, sizeof(int64_t) * (size_t)n_bounds, hipMemcpyHostToDevice, c->stream));
  const size_t ns = (size_t)gtx::adjacent_spans(n);
  HIPCHK(c, c->gapCount.reserve(ns)); HIPCHK(c, c->gapBase.reserve(ns + 1));
  if (!c->gapInfo) HIPCHK(c, c->gapInfo.alloc(1));
  if (!c->gapHost) HIPCHK(c, c->gapHost.alloc(1));
  return GTX_OK;
}

static int gaps_enqueue(gtx_ctx *c, const void *d_tri, int64_t n, int32_t n_bounds, int64_t capacity, void *d_owner, void *d_start, void *d_stop)
{
  HIPCHK(c, gtx::launch_gaps((const int *)d_tri, n, c->gapBounds.get(), n_bounds, capacity, c->gapCount.get(), c->gapBase.get(), c->gapInfo.get(), (unsigned *)d_owner,
                             (int *)d_start, (int *)d_stop, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->gapHost.get(), c->gapInfo.get(), sizeof(gtx::GapInfo), hipMemcpyDeviceToHost, c->stream));
  return GTX_OK;
}

int gtx_gaps_device(gtx_ctx *c, const void *d_triples, int64_t n, const int64_t *bounds, int32_t n_bounds, int64_t capacity, void *d_owner, void *d_start, void *d_stop,
                    gtx_gaps_info *info)
{
  if (!c) return GTX_E_ARG;
  if (int rc = gaps_prepare(c, "gtx_gaps_device", d_triples, n, bounds, n_bounds, capacity, d_owner, d_start, d_stop, info)) return rc;
  if (n == 0) return GTX_OK;
  if (int rc = gaps_enqueue(c, d_triples, n, n_bounds, capacity, d_owner, d_start, d_stop)) return rc;
  c->gapPending = info;
  return GTX_OK;
}

int gtx_gaps(gtx_ctx *c, const int32_t *triples, int64_t n, const int64_t *bounds, int32_t n_bounds, int64_t capacity, uint32_t *owner_out, int32_t *start_out,
             int32_t *stop_out, gtx_gaps_info *info)
{
  if (!c) return GTX_E_ARG;
  if (int rc = gaps_prepare(c, "gtx_gaps", triples, n, bounds, n_bounds, capacity, owner_out, start_out, stop_out, info)) return rc;
  if (n == 0) return GTX_OK;
  const size_t m = (size_t)n, cap = (size_t)std::max<int64_t>(capacity, 1);
  HIPCHK(c, c->adjTri.reserve(3 * m)); HIPCHK(c, c->gapOwner.reserve(cap)); HIPCHK(c, c->gapStart.reserve(cap)); HIPCHK(c, c->gapStop.reserve(cap));
  HIPCHK(c, hipMemcpyAsync(c->adjTri.get(), triples, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, c->stream));
  if (int rc = gaps_enqueue(c, c->adjTri.get(), n, n_bounds, capacity, c->gapOwner.get(), c->gapStart.get(), c->gapStop.get())) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const gtx::GapInfo &h = c->gapHost.get()[0];
  info->n_gaps = h.nGaps; info->first_bad = h.firstBadOut; info->bad_kind = h.badKind;
  const size_t g = (size_t)std::min<int64_t>(h.nGaps, capacity);
  if (g) {
    HIPCHK(c, hipMemcpyAsync(owner_out, c->gapOwner.get(), sizeof(uint32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(start_out, c->gapStart.get(), sizeof(int32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(stop_out, c->gapStop.get(), sizeof(int32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GTX_OK;
}

// ---------------------------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------------------------
int gtx_profile_enable(gtx_ctx *c, int on)
{
  if (!c || on < 0) return GTX_E_ARG;
  c->prof = on != 0; c->profEvery = on > 1 ? on : 1; c->profCalls = 0; c->profSeq = 0; c->profThis = false;
  return GTX_OK;
}

int gtx_profile_read(gtx_ctx *c, int back, float *msKernel, float *msTotal)
{
  if (!c) return GTX_E_ARG;
  if (back < 0 || back >= gtx_ctx::kProfSlots || back >= c->profCalls) return fail(c, GTX_E_STATE, "gtx_profile_read: no such profiled call");
  HIPCHK(c, hipSetDevice(c->device));
  hipEvent_t *ev = c->evRing[(c->profCalls - 1 - back) % gtx_ctx::kProfSlots];
  const bool kernelOnly = c->profEvery > 1;
  HIPCHK(c, hipEventSynchronize(ev[kernelOnly ? 2 : 3]));
  float a = 0, b = 0;
  HIPCHK(c, hipEventElapsedTime(&a, ev[1], ev[2]));
  if (kernelOnly) b = a; else HIPCHK(c, hipEventElapsedTime(&b, ev[1], ev[3]));
  if (msKernel) *msKernel = a;
  if (msTotal) *msTotal = b;
  return GTX_OK;
}

int gtx_profile_last(gtx_ctx *c, float *msKernel, float *msTotal) { return gtx_profile_read(c, 0, msKernel, msTotal); }

int gtx_profile_count(gtx_ctx *c) { return c ? (int)std::min<long long>(c->profCalls, gtx_ctx::kProfSlots) : 0; }

} // extern "C"
