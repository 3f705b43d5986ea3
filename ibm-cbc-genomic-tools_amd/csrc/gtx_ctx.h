// gtx_ctx.h -- the context behind the C ABI of include/gtx.h, private to the host side of the library: gtx_capi.hip (context, reference
// set, count, coverage, the group's hooks, profiling) and gtx_api_join.hip / gtx_api_scan.hip / gtx_api_text.hip / gtx_api_link.hip
// (one family of entry points each).  struct gtx_ctx holds the core fields and one named struct per family; a family's functions touch
// the core and their own struct, and a field that another family reads says so.  Below the context: the helpers that cross from one
// family to another.  Everything here is hidden from the library's exports.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "gtx.h"
#include "gtx_kernels.h"
#include "gtx_pairs.h"
#include "gtx_link.h"
#include "gtx_adjacent.h"
#include "gtx_internal.h"

namespace gtx { struct JoinInfo; struct SignalInfo; struct RewriteRec; struct WindowsRec; struct ConvertRec; struct BlocksRec; }   // (gtx_join.h, gtx_signal.h, gtx_rewrite.h, gtx_windows.h, gtx_convert.h, gtx_blocks.h: held here by pointer only)

#pragma GCC visibility push(hidden)

typedef unsigned long long u64;

namespace gtxhost {

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

// whose block of text a slot holds between the family's _text call and its _result call (gtx_api_textblock.h)
enum TextPending { TEXT_NONE, TEXT_SUBSET, TEXT_REWRITE, TEXT_WINDOWS, TEXT_CONVERT, TEXT_BLOCKS };

// a block of region text tokenised on the device (gtx_count_add_text)
struct TextSlot {
  DevBuf<char> text; DevBuf<unsigned> seg;
  DevBuf<unsigned> nl; DevBuf<int> tri, w;                    // w (made last) holds the lines these are made for
  DevBuf<int> tri2; DevBuf<unsigned> blk; DevBuf<int> w2;      // ... w2 those of the strand-aware outputs
  DevBuf<int> flag; PinBuf<int> hostFlag; PinBuf<char> pin, seam; DevBuf<unsigned long long> sum;
  hipEvent_t evParsed = nullptr, evConsumed = nullptr, evCopied = nullptr; bool busy = false;
  // the family whose block the slot holds, its result not fetched yet: a slot holds one block, so the next family's block ends it
  TextPending pending = TEXT_NONE;
  // gtx_subset_text: the lines' hits, the tiles' kept bytes / lines, the kept text and its totals on the host
  DevBuf<unsigned> hits; DevBuf<unsigned long long> tile; DevBuf<char> out; PinBuf<unsigned long long> hostTotal;
  // gtx_rewrite_text: the lines' records, the tiles' bytes | lines and their prefixes (`out` and `hostTotal` as for the subset)
  DevBuf<gtx::RewriteRec> rwRec; DevBuf<unsigned> rwTile; DevBuf<long long> rwBase;
  // gtx_windows_text: the lines' records, the tiles' windows | bytes and their prefixes, the lines' bases (windows | bytes); what
  // gtx_windows_result needs of the call to render the block (`hostTotal`: the block's windows and bytes)
  DevBuf<gtx::WindowsRec> wnRec; DevBuf<unsigned long long> wnTile; DevBuf<long long> wnBase, wnLine;
  long long wnSize = 0, wnStep = 0; int wnSmall = 0; size_t wnBytes = 0; unsigned wnLines = 0;
  // gtx_convert_text: the lines' records, the tiles' bytes and their prefix (`out` and `hostTotal` as for the subset)
  DevBuf<gtx::ConvertRec> cvRec; DevBuf<unsigned> cvTile; DevBuf<long long> cvBase;
  // gtx_blocks_text: the lines' records, the tiles' bytes | printed lines and their prefixes, split's bases of the lines (printed
  // lines; bytes); what gtx_blocks_result needs of the call to render the block (`hostTotal`: the block's bytes and printed lines)
  DevBuf<gtx::BlocksRec> blRec; DevBuf<unsigned> blTile, blLineOut; DevBuf<long long> blBase, blLineByte;
  int blKind = 0, blSelect = 0, blStrand = 0; size_t blBytes = 0; unsigned blLines = 0;
};

// What a device call found, on its way to the caller's struct: the info block the kernels write, its page-locked copy, and the
// struct of the caller whose call has been enqueued but not synchronised (gtx_sync, or the family's next call, delivers it).
// publish(block, struct) is the field copy, one overload per kind of info.
inline void publish(const gtx::LinkInfo &h, gtx_link_info *o) { o->n_groups = h.nGroups; o->first_unsorted = h.firstUnsortedOut; }
inline void publish(const gtx::AdjInfo &h, gtx_adjacent_info *o) { o->first_unsorted = h.firstUnsortedOut; o->n_inclusions = h.nInclusions; o->n_overlaps = h.nOverlaps; }
inline void publish(const gtx::GapInfo &h, gtx_gaps_info *o) { o->n_gaps = h.nGaps; o->first_bad = h.firstBadOut; o->bad_kind = h.badKind; }

template <class Dev, class Pub> struct InfoMail {
  DevBuf<Dev> dev; PinBuf<Dev> host; Pub *pending = nullptr;
  // both blocks allocated once
  hipError_t ready() { hipError_t e = dev ? hipSuccess : dev.alloc(1); if (e == hipSuccess && !host) e = host.alloc(1); return e; }
  // device block -> page-locked copy, enqueued
  hipError_t post(hipStream_t s) { return hipMemcpyAsync(host.get(), dev.get(), sizeof(Dev), hipMemcpyDeviceToHost, s); }
  // the copy has arrived (the caller has waited for the stream): into the pending struct, if there is one
  void deliver() { if (pending) { publish(host.get()[0], pending); pending = nullptr; } }
};

// the overlap join's offsets / scan / pair buffers of the host-buffer entry, its queries; per-query hits, the pair offsets' and the
// annotate pass' host entries.  The subset of text blocks (gtx_subset_text, gtx_api_text.hip) counts its lines' hits through `info`
// and `off` too: it is the join's count walk over tokenised lines.
struct JoinState {
  DevBuf<long long> off, part, cut; DevBuf<int> pairs, scratch; DevBuf<unsigned> big;
  DevBuf<int> reads; DevBuf<int2> qBlk, qIv;
  DevBuf<gtx::JoinInfo> info;
  DevBuf<unsigned> hitsOut;             // gtx_query_hits: a batch's hits
  int64_t buffer = 1ll << 26;           // pairs per device chunk of gtx_join (gtx_set_join_buffer)
  DevBuf<long long> offInv, offOut, offCnt, offPart; DevBuf<int8_t> offQStrand;   // the pair offsets' host entry
  DevBuf<long long> annCnt, annVal; DevBuf<int> annRef;   // the annotate pass' host entry: a chunk's kept offsets, values and ordinals
};

// the signal bins' info block, the host entry's bins and weights
struct SignalState { DevBuf<gtx::SignalInfo> info; DevBuf<unsigned long long> bins; DevBuf<long long> w; };

// gtx_scan_begin .. gtx_scan_end: the open scan's geometry and what its batches have added so far
struct ScanOpen { bool open = false, weighted = false; gtx::ScanArgs a; std::vector<int32_t> classLen; int64_t extent = 0; char prep = '1'; uint32_t flags = 0;
                  DevBuf<unsigned long long> labelSum; };

// scan state
struct ScanState {
  DevBuf<u64> micro;
  DevBuf<long long> tab;
  std::vector<long long> key;           // geometry the tables on the device were built for
  int64_t totalWindows = 0, totalMicro = 0, totalTiles = 0;
  // unsorted reads: bucket tables over the positions of a scan geometry (scan_bucket_tables), the parts they are counted in
  BucketTables bkt; DevBuf<gtx::ScanPart> parts; int nParts = 0; std::vector<long long> bktKey; DevBuf<gtx::DevInfo> info;
  // owner-computes scan of sorted reads (gtx_scanown.hip): block table for the current tile, bounds scratch, give-up flag;
  // reads of a host-buffer call held resident for its single launch (the two events are made and destroyed with the context)
  int64_t ownBlocks = 0; DevBuf<long long> bounds; DevBuf<int> flag;
  DevBuf<char> resReads; DevBuf<int> resWeights; hipEvent_t evRes[2] = {nullptr, nullptr};
  // the open scan.  The text feed (gtx_scan_add_text, gtx_api_text.hip) reads it: a block of text is one more batch of that scan
  ScanOpen cur;
  // gtx_scan_end_keep: window vectors that stay in HBM (their extents beside them)
  DevBuf<u64> kept[GTX_SCAN_KEEP_SLOTS]; int64_t keptLen[GTX_SCAN_KEEP_SLOTS] = {};
};

// What the tile compactions (gtx_compact.h: window selection, window filter, peak candidates) share: the passes' tile counts and
// bases, the total on the host, and the host entries' results -- ordinals, and the rows beside them in a buffer sized in bytes.  One
// set serves all of them because each of their six entry points ends in a stream sync before it returns and none keeps a result on
// the device for a later call.
struct CompactState { DevBuf<unsigned> count; DevBuf<long long> base, ord; DevBuf<char> rows; PinBuf<long long> total; };

// the window selection's tables
struct SelectState { DevBuf<int> tab; };

// the window filter: the region set gtx_window_refs prepared (its triples as given, keyed and sorted; starts, running maxima of the
// stops, the classes' first regions; the classes that have windows in offset order) with the geometry it was prepared for
struct FilterState {
  bool set = false; int nClasses = 0, nBlk = 0, step = 0, size = 0; int64_t extent = 0;
  DevBuf<int> tri, keyed, sorted, start, runmax, first, blkCls; DevBuf<unsigned> order, bad; DevBuf<long long> blkOff, blkEnd;
};

// the line renderer (gtx_lines.hip): the layout gtx_lines_layout uploaded with what the host keeps of it, the passes' per-tile lines
// and bytes with their sums, the all-ones word, the totals of two ranges in flight on the host (lines, bytes, end word each), and the
// streaming entries' two device and two page-locked text buffers with the events of their copies
struct LinesState {
  bool set = false; int nBlocks = 0, maxLine = 0; int64_t total = 0, step = 0, size = 0, chunkBytes = 64ll << 20;
  DevBuf<long long> blockOff; DevBuf<int> nameOff; DevBuf<char> names, strand;
  DevBuf<unsigned> tileLines, tileBytes; DevBuf<long long> baseLines, baseBytes; DevBuf<unsigned long long> endWord;
  PinBuf<unsigned long long> totals;
  DevBuf<char> text[2]; PinBuf<char> pin[2]; hipEvent_t evCopied[2] = {nullptr, nullptr};
  ~LinesState() { for (int k = 0; k < 2; k++) if (evCopied[k]) (void)hipEventDestroy(evCopied[k]); }
};

// link: the scans' per-tile values and break bit map, the info block and its page-locked copy (handed to the caller's struct by
// gtx_sync after a device call), the host entry's inputs and group records
struct LinkState {
  DevBuf<int2> agg, prefix; DevBuf<u64> bits; DevBuf<unsigned> heads; DevBuf<long long> base;
  InfoMail<gtx::LinkInfo, gtx_link_info> mail;
  DevBuf<int> tri, stop; DevBuf<long long> vals, val; DevBuf<unsigned> head, cnt;
  // gtx_link_text_begin .. _end: the input collected on the device block by block, the strands beside it, the heads' keys
  bool textOpen = false; int64_t textN = 0, textCap = 0; int textChrom = 0, textByStrand = 0;
  DevBuf<int> textTri; DevBuf<unsigned char> minus; DevBuf<int2> headKey;
};

// the neighbour passes (gtx_adjacent / gtx_gaps): per-tile sums, per-span gap counts and bases, the class bounds, the info blocks
// and their page-locked copies (handed over like link's), the host entries' inputs and outputs
struct NeighbourState {
  DevBuf<uint2> sums; DevBuf<unsigned> gapCount; DevBuf<long long> gapBase, gapBounds;
  InfoMail<gtx::AdjInfo, gtx_adjacent_info> adj;
  InfoMail<gtx::GapInfo, gtx_gaps_info> gap;
  DevBuf<int> tri;                      // the host entries' triples on the device: gtx_adjacent's and gtx_gaps' alike (one call at a time)
  DevBuf<int> gapStart, gapStop; DevBuf<unsigned char> minus; DevBuf<long long> dist; DevBuf<unsigned> gapOwner;
};

// staging for the host-buffer entry points: two device slots fed from two pinned host slots by a copy stream, so that
// the host->device copy of batch i+1 runs under the kernels of batch i (stage_batches below).  Every family's host-buffer entry
// goes through it: the copy stream is what they and gtx_sync wait for, the scans' resident reads and the text feed borrow the pinned
// slots' machinery (copyThreads, directPending).  Stream and events are made and destroyed with the context.
struct Staging {
  hipStream_t copyStream = nullptr;
  DevBuf<char> dev[2]; DevBuf<int> devW[2];       // (12 bytes per read)
  PinBuf<char> pin[2];                            // bytes per slot
  hipEvent_t evCopied[2] = {nullptr, nullptr}, evConsumed[2] = {nullptr, nullptr}; bool slotBusy[2] = {false, false};
  long long seq = 0; bool directPending = false;  // a DMA may still be reading the page-locked buffer of the last call
  int copyThreads = 8;                  // host threads that move a pageable batch into the pinned slot (GTX_COPY_THREADS)
};

// region text tokenised on the device (gtx_count_add_text): two blocks in flight, the names' tables
struct TextState {
  TextSlot slot[2];
  long long seq = 0;
  DevBuf<int> table; DevBuf<char> names; unsigned mask = 0, blobLen = 0;
  std::string blob;                                   // the chromosome names the device tables were built from
  DevBuf<long long> chromLen; std::vector<long long> h_chromLen;   // gtx_rewrite_text, bounds: the lengths per class, and what was uploaded
  // gtx_windows_result: two device and two page-locked buffers for the ranges of a block's windows in flight, the events of their
  // copies, the ranges' bytes on the device and on the host
  DevBuf<char> wnOut[2]; PinBuf<char> wnPin[2]; hipEvent_t wnCopied[2] = {nullptr, nullptr};
  DevBuf<unsigned long long> wnRange; PinBuf<unsigned long long> wnHostRange;
  // gtx_blocks_result: the printed text of the block being fetched, on the device and page-locked
  DevBuf<char> blOut; PinBuf<char> blPin;
  ~TextState() { for (int k = 0; k < 2; k++) if (wnCopied[k]) (void)hipEventDestroy(wnCopied[k]); }
};

// measurement (prof_begin / prof_mark / prof_end below)
struct Profile {
  static constexpr int kSlots = 64;     // ring: the last 64 profiled calls can be read back
  bool on = false; long long calls = 0;
  int every = 1; long long seq = 0; bool profThis = false;   // gtx_profile_enable(N >= 2): kernel-only events on every N-th call
  hipEvent_t ring[kSlots][4] = {};
  hipEvent_t *ev = ring[0];
};

} // namespace gtxhost

using namespace gtxhost;   // (a private header: the translation units that include it are the host side these names were made for)

#pragma GCC visibility pop    // the struct the C ABI names, as visible as that name
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

  DevBuf<gtx::DevInfo> d_info;          // 2 blocks: the finalize of one call resets the block of the next
  int infoCur = 0;
  PinBuf<gtx::DevInfo> h_info;          // [0] = readback, [1] = init pattern

  DevBuf<u64> out;
  DevBuf<char> scratch;                 // gtxi_scratch

  // streaming count (begin/add/end)
  bool streamOpen = false; int64_t streamSeen = 0; int32_t streamLast[2] = {0, 0};
  int64_t seamUnsorted = INT64_MAX;    // first order violation found at a seam between batches (host-side check)

  int64_t batchReads = 8ll << 20;       // reads per device batch of the host-buffer entry points (96 MiB of triples: ~2 ms of PCIe)
  int chunksPerWave = 0;                // 0 = choose per call from the number of reads
  int64_t waveSlots = 8192;             // resident waves of the device (CUs x 32)

  // one struct per family of entry points
  Staging stage;
  JoinState join;
  SignalState sig;
  ScanState scan;
  CompactState cmp;
  SelectState sel;
  FilterState flt;
  LinesState lines;
  TextState text;
  LinkState link;
  NeighbourState nbr;
  Profile prof;
};
#pragma GCC visibility push(hidden)

#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return GTX_E_HIP; } } while (0)

inline int fail(gtx_ctx *c, int code, const char *msg) { c->err = msg; return code; }

// b = the n elements of v, in a buffer of exactly n
template <class T> hipError_t upload(DevBuf<T> &b, const T *v, size_t n)
{
  hipError_t e = b.alloc(n);
  return e == hipSuccess ? hipMemcpy(b.get(), v, sizeof(T) * n, hipMemcpyHostToDevice) : e;
}

// The bracket of a profiled entry point: begin decides whether this call is profiled and picks its slot of the ring, mark(k) records
// event k of a profiled call (1: before the kernels, 2: behind them), end records event 3 -- only when every call is profiled -- and
// counts the call.  An entry point that returns on an error in between leaves the counters where they were.
inline void prof_begin(gtx_ctx *c)
{
  c->prof.profThis = c->prof.on && (c->prof.every <= 1 || (c->prof.seq++ % c->prof.every) == 0);
  if (c->prof.profThis) c->prof.ev = c->prof.ring[c->prof.calls % Profile::kSlots];
}
inline hipError_t prof_mark(gtx_ctx *c, int k, hipStream_t s) { return c->prof.profThis ? hipEventRecord(c->prof.ev[k], s) : hipSuccess; }
inline hipError_t prof_end(gtx_ctx *c, hipStream_t s)
{
  if (!c->prof.profThis) return hipSuccess;
  const hipError_t e = c->prof.every <= 1 ? hipEventRecord(c->prof.ev[3], s) : hipSuccess;
  if (e == hipSuccess) c->prof.calls++;
  return e;
}

// ---------------------------------------------------------------------------------------------
// helpers that cross from one family to another (defined in the file named; their comments are there)
// ---------------------------------------------------------------------------------------------
// who counts: any entry point, a group member (its classes only: CountArgs::owned), or a member's call on one of the group's streams
// (gtxi_count_device_share_async)
enum CountCall { COUNT_ANY, COUNT_SHARE, COUNT_SHARE_ASYNC };

// gtx_capi.hip: the reference side
int make_hist_set(gtx_ctx *c, HistSet &h, int64_t histLen);
int make_place_table(gtx_ctx *c, const std::vector<int32_t> &seg, const std::vector<int32_t> &arrA, const std::vector<int32_t> &arrB,
                     int nClasses, int64_t nv, PlaceTable &out);
int build_bucket_tables(gtx_ctx *c, BucketTables &t, BucketCuts &k, int nClasses, bool sync = false);
// gtx_capi.hip: count
gtx::CountArgs count_args(gtx_ctx *c, const HistSet &h, uint32_t flags, int64_t nReads, int64_t indexBase = 0, CountCall who = COUNT_ANY,
                          bool hist32 = false);
int partition_plan(gtx_ctx *c, const BucketTables &t, int64_t n, int nClasses, bool weighted, gtx::BucketPlan *p, gtx::BucketWork *w, bool *yes);
int launch_unsorted(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, const gtx::CountArgs &a);
int ref_columns(gtx_ctx *c);
int merge_prepare(gtx_ctx *c, uint32_t flags, int mode);
int pairs_batch(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n);
int merge_batch(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n);
int merge_end(gtx_ctx *c, void *d_out);
// gtx_capi.hip: host buffers -> device
bool is_pinned(const void *p);
void parallel_copy(char *dst, const char *src, size_t bytes, int threads);
int stage_reserve(gtx_ctx *c, size_t nReads, bool weights, bool pinnedSlots);
int ensure_out(gtx_ctx *c, size_t n);
// gtx_capi.hip: the pair corrections, coverage
bool blocks_monotone(const int32_t *b, int64_t cnt);
gtx::RegionBlocks ref_blocks(const gtx_ctx *c);
int cover_launch(gtx_ctx *c, const void *dR, const int *dW, int64_t n, int64_t indexBase, uint32_t flags, bool unsorted);
bool host_reads_look_unsorted(const int32_t *tri, int64_t n);
// gtx_api_join.hip
int join_prepare(gtx_ctx *c);
int join_mode(gtx_ctx *c, uint32_t flags);
// gtx_api_scan.hip
int scan_hist_any(gtx_ctx *c, const void *dR, const int *dW, int64_t n, const gtx::ScanArgs &a, const int32_t *classLen, bool unsorted);
// gtx_api_text.hip (the handshake around it of the families that hand text back: gtx_api_textblock.h)
int text_stage(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, bool grouped, int scanRules,
               unsigned long long *labelSum, int format, TextSlot **tp, int *ticket, bool *empty);

// Streams reads[0..n) (and weights) through the device in batches; launch(d_reads, d_weights, cnt, off) enqueues the
// kernels of one batch on the context's stream.  Returns with everything enqueued; the caller's buffers are free again
// when the function returns unless they are page-locked, in which case they must stay untouched until the context's next
// host-buffer call, gtx_*_end or gtx_sync has returned.
template <class Launch>
int stage_batches(gtx_ctx *c, const int32_t *reads, const int32_t *weights, int64_t n, Launch launch)
{
  if (c->stage.directPending) { HIPCHK(c, hipStreamSynchronize(c->stage.copyStream)); c->stage.directPending = false; }   // the previous call's page-locked source is free now
  if (n <= 0) return GTX_OK;
  const int64_t batch = c->batchReads;
  const bool direct = is_pinned(reads) && (!weights || is_pinned(weights));
  c->stage.directPending = direct;
  int rc = stage_reserve(c, (size_t)std::min<int64_t>(n, batch), weights != nullptr, !direct); if (rc) return rc;
  for (int64_t off = 0; off < n; off += batch) {
    const int64_t cnt = std::min(batch, n - off);
    const int slot = (int)(c->stage.seq++ & 1);
    if (c->stage.slotBusy[slot]) {
      // the pinned slot is free once its DMA is done; the device slot once the kernels that read it are
      if (!direct) HIPCHK(c, hipEventSynchronize(c->stage.evCopied[slot]));
      HIPCHK(c, hipStreamWaitEvent(c->stage.copyStream, c->stage.evConsumed[slot], 0));
    }
    const char *srcR = (const char *)(reads + 3 * off), *srcW = (const char *)(weights ? weights + off : nullptr);
    if (!direct) {
      parallel_copy(c->stage.pin[slot].get(), srcR, (size_t)cnt * 12, c->stage.copyThreads);
      if (weights) parallel_copy(c->stage.pin[slot].get() + (size_t)cnt * 12, srcW, (size_t)cnt * 4, c->stage.copyThreads);
      srcR = c->stage.pin[slot].get(); srcW = c->stage.pin[slot].get() + (size_t)cnt * 12;
    }
    HIPCHK(c, hipMemcpyAsync(c->stage.dev[slot].get(), srcR, (size_t)cnt * 12, hipMemcpyHostToDevice, c->stage.copyStream));
    if (weights) HIPCHK(c, hipMemcpyAsync(c->stage.devW[slot].get(), srcW, (size_t)cnt * 4, hipMemcpyHostToDevice, c->stage.copyStream));
    HIPCHK(c, hipEventRecord(c->stage.evCopied[slot], c->stage.copyStream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->stage.evCopied[slot], 0));
    rc = launch(c->stage.dev[slot].get(), weights ? c->stage.devW[slot].get() : nullptr, cnt, off); if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->stage.evConsumed[slot], c->stream));
    c->stage.slotBusy[slot] = true;
  }
  return GTX_OK;
}

// the envelopes of the regions `pick` selects, per class in the order of their starts, with the running and the per-64 maxima
// of their ends.  Which regions take part at all follows gtx_set_refs (placeholders and, under the bin index's rules, regions
// with start > stop or stop <= 0 never match); under the sorted merge's rules every region with a class does, inverted or not:
// the envelope test below is the merge's own (CalcDirection == 0, genomic_intervals.cpp:1225-1236).
template <class Pick>
int build_pair_index(gtx_ctx *c, RefExtras::PairIdx *out, Pick pick)
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

#pragma GCC visibility pop
