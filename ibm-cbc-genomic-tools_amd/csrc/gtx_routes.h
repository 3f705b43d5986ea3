// gtx_routes.h -- which kernels a call takes: every shape rule of the count, coverage and scan paths as a pure function of the
// shape and the knobs, with the constants they turn on.  Host only, no HIP: the library calls these (gtx_capi.hip, gtx_api_scan.hip, launch_finalize),
// and the CPU suite calls them at their thresholds through `gtx_packtool route`.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

namespace gtx {

constexpr int kTileShift = 10;                // finalize scan tile = 1024 histogram slots
constexpr int kTile = 1 << kTileShift;
constexpr int kChainMaxTiles = 512;           // the chained one-launch finalize up to this many tiles (finalize_scan_chained_kernel: every block's wait is short)
constexpr int kLocalScanMaxTiles = 2048;      // 2 x 2048 offsets in the gather's LDS: 16 KB with 32-bit slots, 32 KB with 64-bit ones
constexpr long long kTileSumsMaxReads = 1 << 20;       // the streaming kernel keeps the tile sums below this many reads in one launch
constexpr long long kFlipRegions = 256, kFlipReads = 4;   // the all-boundaries-at-once walk from 4 boundaries per 256 reads and array
constexpr long long kBucketMinReads = 1 << 18;         // reads in no order: the partition path from this many reads in one batch (GTX_BUCKET_MIN_READS, per context)
constexpr int kScanBktMaxBuckets = 4096, kScanBktMaxClasses = 2048;   // scan partition tables only up to these
constexpr long long kScanBktMinPer = 16384;   // micro-windows per scan bucket, at least
constexpr long long kScanBktDefault = 2000;   // buckets a scan geometry is cut into (100 M shuffled reads, -d 25: 500 -> 2.77 ms, 1000 -> 2.30, 2000 -> 2.15, 3000 -> 2.10)

inline int scan_tiles(long long len) { return (int)((len + kTile - 1) / kTile); }

// The environment overrides that change a route.  Per PROCESS: the library reads them once, at the first call that asks (route_knobs).
// (GTX_BUCKET_MIN_READS, GTX_LOCAL_SCAN_MAX_TILES, GTX_CHUNKS_PER_WAVE, GTX_BATCH_READS and GTX_COPY_THREADS are per CONTEXT: gtx_create
// reads them, and the rules below take them as plain arguments.)
struct RouteKnobs {
  bool chained = true;                    // GTX_CHAINED_SCAN=0: never the chained finalize
  int chainMax = kChainMaxTiles;          // GTX_CHAIN_MAX_TILES
  long long partMaxHist = INT64_MAX;      // GTX_PART_MAX_HIST: the longest histogram whose tile sums a large launch leaves to the finalize step
  bool hist32 = true;                     // GTX_HIST32=0: 64-bit histogram slots always
  bool flipForced = false, flipOn = false;   // GTX_FLIP=0|1
  bool weightedFast = true;               // GTX_WEIGHTED_FAST=0: weighted coverage through the general per-chunk code
  long long scanBuckets = kScanBktDefault;   // GTX_SCAN_BUCKETS (> 0)
  bool scanOwn = true, scanFused = true;  // GTX_SCAN_OWN=0, GTX_SCAN_FUSED=0
  static RouteKnobs from_env()
  {
    auto off = [](const char *name) { const char *v = getenv(name); return v && atoi(v) == 0; };
    RouteKnobs k;
    k.chained = !off("GTX_CHAINED_SCAN"); k.hist32 = !off("GTX_HIST32"); k.weightedFast = !off("GTX_WEIGHTED_FAST");
    k.scanOwn = !off("GTX_SCAN_OWN"); k.scanFused = !off("GTX_SCAN_FUSED");
    if (const char *v = getenv("GTX_CHAIN_MAX_TILES")) k.chainMax = atoi(v);
    if (const char *v = getenv("GTX_PART_MAX_HIST")) k.partMaxHist = atoll(v);
    if (const char *v = getenv("GTX_FLIP")) { k.flipForced = true; k.flipOn = atoi(v) != 0; }
    if (const char *v = getenv("GTX_SCAN_BUCKETS")) if (atoll(v) > 0) k.scanBuckets = atoll(v);
    return k;
  }
};
inline const RouteKnobs &route_knobs() { static const RouteKnobs k = RouteKnobs::from_env(); return k; }

// The finalize step of a count call (launch_finalize).  nb: the tiles of the histograms; nbRun: the tiles this call scans -- a group
// member's listed ones, nb otherwise.  The chained kernel launches a block per tile it RUNS, the local scan's gather keeps an offset per
// tile there IS (all of them, in LDS): hence nbRun in one rule and nb in the other.  Tile sums kept by the streaming kernel: finalize_scan
// + gather_hits; not kept: one launch for tile sums + scan (finalize_scan_chained_kernel, needs the chain flags) + gather_hits, or a
// tile-local scan and a gather that adds the tiles' offsets (finalize_local + gather_hits_local, needs the totals), or tile_sums first.
enum FinalizeRoute { FIN_GATHER_ONLY, FIN_SUMS_KEPT, FIN_CHAINED, FIN_LOCAL, FIN_SUMS_SCAN };
inline FinalizeRoute finalize_route(int nb, int nbRun, bool tileSumsValid, bool haveChain, bool haveTotals, int localMaxTiles, const RouteKnobs &k)
{
  if (nbRun <= 0) return FIN_GATHER_ONLY;
  if (tileSumsValid) return FIN_SUMS_KEPT;
  if (haveChain && k.chained && nbRun <= k.chainMax) return FIN_CHAINED;
  if (haveTotals && nb <= std::min(localMaxTiles, kLocalScanMaxTiles)) return FIN_LOCAL;
  return FIN_SUMS_SCAN;
}

// Large batches: the streaming kernel leaves the per-tile sums alone and the finalize step rebuilds them from the
// histograms (tile_sums_kernel, one pass over 16 B per region: 6 us at 1 M regions).  Keeping them up to date costs two
// more atomics and a wave scan per window flush -- 100 M reads x 1 M regions: kernel 0.218 -> 0.207 ms, step 0.253 ->
// 0.248 ms; with few regions every wave hits the same handful of counters and the same-address atomics serialise
// (10 k regions: 0.28 -> 0.19 ms; a group member's 1/8 of 100 M reads over its 3 chromosomes: 0.041 -> 0.103 ms).  Small batches
// keep the sums (no extra launch).  GTX_PART_MAX_HIST=0 restores them.
inline bool keeps_tile_sums(long long histLen, long long nReads, const RouteKnobs &k) { return !(histLen <= k.partMaxHist && nReads >= kTileSumsMaxReads); }

// dense references (>= 4 boundaries per 256 reads and array): all boundaries of a window at once instead of the
// per-boundary loop (100 M reads x 4 M regions: 0.41 -> 0.28 ms; at 1 M regions the loop is 3 % faster).  GTX_FLIP=0|1 forces.
inline bool flip_walk(long long regions, long long nReads, const RouteKnobs &k) { return k.flipForced ? k.flipOn : regions * kFlipRegions >= kFlipReads * std::max<long long>(nReads, 1); }

// 32-bit histogram slots: a call that is ONE launch of the streaming kernel over unweighted reads, fewer than 2^32 of them (no slot or prefix can pass that)
inline bool hist32_slots(bool singleUnweightedLaunch, long long nReads, const RouteKnobs &k) { return singleUnweightedLaunch && k.hist32 && nReads < (1ll << 32); }

// span of one wave of the streaming count kernel, in 64-read chunks (forced > 0: GTX_CHUNKS_PER_WAVE): long enough to amortise the
// window placement at its start, short enough that the grid has >= 3 rounds of the 8192 wave slots of the chip (256 CUs x 32 waves)
// and that the waves resident at one time read a compact piece of the stream (100 M reads: flat from 48 to 64 chunks, +3 % at 96,
// +12 % at 192 = one round; 1 G reads: 1.74 ms at 48, 1.76 at 64-96, 1.82 at 128; the bare load pattern behaves the same,
// scripts/membench.hip).  Launches of one to three rounds -- a group member's share of 100 M reads -- take 16 chunks per wave from a
// full round of 16-chunk spans on: the start of a span is paid once per 16 chunks instead of 8, 0.039 -> 0.034 ms for 12.9 M reads
// (scripts/r04_share.sh).  Rounded up to the 4 reads a lane takes per step.
inline int count_chunks_per_wave(long long nReads, long long waveSlots, int forced)
{
  const long long nChunks = (nReads + 63) >> 6;
  const int cpw = forced > 0 ? forced : (int)std::min<long long>(56, std::max<long long>(nChunks >= 16 * waveSlots ? 16 : 8, nChunks / 24576));
  return (cpw + 3) / 4 * 4;
}
// coverage: as above, a little longer (the start of a span costs more here: 100 M reads: 0.55 ms at 16 chunks, 0.44 at 32, 0.382 at 56,
// 0.374 at 64, 0.383 at 96)
inline int cover_chunks_per_wave(long long nReads, int forced)
{
  const int cpw = forced > 0 ? forced : (int)std::min<long long>(64, std::max<long long>(8, ((nReads + 63) >> 6) / 24576));
  return (cpw + 3) / 4 * 4;
}

// reads in no particular order: a batch worth partitioning into buckets (below, the per-read search / the streaming and general
// kernels serve; the partition pass indexes its reads in 31 bits)
inline bool partition_worth(long long n, long long bucketMinReads) { return n >= bucketMinReads && n < (1ll << 31); }

// scan partition tables: micro-windows per bucket -- about knobs.scanBuckets buckets in all, kScanBktMinPer micro-windows each at the
// least, in whole parts of partBins (every part of a bucket reads all of the bucket's chunks, a short last one as well)
inline long long scan_bucket_per(long long totalMicro, int partBins, const RouteKnobs &k)
{
  const long long per = std::max(kScanBktMinPer, (totalMicro + k.scanBuckets - 1) / k.scanBuckets);
  return per > partBins ? per / partBins * partBins : per;
}
inline bool scan_bucket_tables_ok(long long nB, int nClasses, long long totalMicro) { return nB > 0 && nB <= kScanBktMaxBuckets && nClasses <= kScanBktMaxClasses && totalMicro < (1ll << 31); }
// sorted scans: the owner-computes pass (gtx_scanown.hip) is tried; scans in no order: the parts of the partition path write their
// windows themselves (no micro-window array, no window pass)
inline bool scan_own_wanted(bool readsSorted, bool prepOne, long long nReads, const RouteKnobs &k) { return readsSorted && prepOne && k.scanOwn && nReads > 0; }
inline bool scan_fused_ok(int comb, int maxComb, long long totalWindows, const RouteKnobs &k) { return k.scanFused && comb <= maxComb && totalWindows > 0; }

} // namespace gtx
