// Tile compaction: the windows of a vector that a rule keeps, written out in window order.  The shape the window selection
// (gtx_select.hip), the window filter (gtx_filter.hip) and the peak candidate selection (gtx_peaks.hip) share; each of them is a
// rule over it.  Reduce-then-scan over fixed tiles, three launches (launch_compact):
//
//   compact_kernel<.., false>  per tile of kCompactTile windows the number kept
//   launch_tile_prefix         exclusive sum of the tile counts in one block (block_exclusive_sum); base[tiles] = the number kept
//   compact_kernel<.., true>   the rule once more; a kept window goes to base[tile] + its rank inside the tile while that is below
//                              the caller's capacity: its ordinal (written here) and what the rule writes beside it.  A tile whose
//                              count is zero, or whose base lies behind the capacity, loads nothing
//
// A tile belongs to one wave: kCompactRows rows of 128 consecutive windows, lane l of a row holding windows 2 l and 2 l + 1, which a
// rule reads from each of its vectors with one 16-byte load (load_pair).  The rank of a kept window inside its tile is the
// wave-uniform count of the rows in front of it plus the popcounts of the row's two ballots below its lane, so the waves of a block
// share nothing.  No block waits for another and none reads what a block of its own launch wrote: every dependency between tiles is
// a kernel boundary.
//
// A rule is a struct passed to the kernels by value.  It derives from CompactRule and supplies
//
//   struct Payload                          what it keeps of one window between the test and the write
//   void load(i, n, Payload &p0, &p1)       windows i and i + 1 (i even) of its vectors, one load_pair each; what lies behind n reads
//                                           as 0.  Both windows at once, because one 16-byte load brings both
//   bool keep(i, const Payload &) const     the test of window i; i < n holds (the kernel tests the bound)
//   void emit(out, g, i, const Payload &)   kept window i has rank g < capacity: row g of the rule's output
//
// and, when it needs them, overrides
//
//   size_t lds_bytes() const (host)         dynamic LDS of a block
//   void block()                            a block's prologue; every wave of the block runs it before it may return
//   kTwoRowsInFlight = true                 whole tiles take a loop without the end test between rows, so that the loads of two rows
//                                           are out together: worth its registers when a row is many loads (the selection, measured)
//   bool tile(tileStart, tileEnd, lane)     a wave's prologue, run by all 64 lanes before any diverges: false = no window of this tile
//                                           can be kept (its count is 0 and none of its windows is loaded).  It may set members for keep
//
// Integer code only: whatever rounds stays with its rule.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_scan.h"

namespace gtx {

constexpr int kCompactThreads = 256, kCompactRows = 8;
constexpr int kCompactTile = 64 * 2 * kCompactRows;                   // windows per wave: kCompactRows rows of two windows per lane
inline long long compact_tiles(long long n) { return (n + kCompactTile - 1) / kCompactTile; }

// The scans over per-tile values run in one block of kPartThreads lanes, each over a run of consecutive tiles with its loads out
// kPartBatch at a time (gtx_scan.h): block_exclusive_sum below, or a first and last pass of the kernel's own around a tile_exclusive.
constexpr int kPartThreads = 1024;
using gtxscan::kPartBatch;

// base [tiles + 1] = the exclusive sums of count [tiles], base[tiles] their total (defined in gtx_select.hip)
hipError_t launch_tile_prefix(const unsigned *tileCount, long long tiles, long long *tileBase, hipStream_t st);
// the same over 64-bit counts, for tiles whose count need not fit 32 bits (the sliding windows' plan, gtx_windows.hip)
hipError_t launch_tile_prefix64(const unsigned long long *tileCount, long long tiles, long long *tileBase, hipStream_t st);

// The body of that scan, for a block of kPartThreads threads with sh [kPartThreads] in LDS: base[k] = count[0] + .. + count[k - 1] for
// k = 0 .. n.  It ends in a barrier: behind it every thread may read base[0 .. n] and sh is free.  COUNT: unsigned, or unsigned long long.
// It keeps its own two turns and LDS ladder and is not gtxscan::run_exclusive_sum: built on that, launch_tile_prefix came out about 0.005 ms
// slower than this in two sessions against the parent's library (profiles/scan_ab.txt), for a reason the ISA does not show.
template <class COUNT>
__device__ __forceinline__ void block_exclusive_sum(const COUNT *__restrict__ count, long long n, long long *__restrict__ base, long long *sh)
{
  typedef long long i64;
  const int tid = threadIdx.x;
  const i64 per = (n + kPartThreads - 1) / kPartThreads, b = min((i64)tid * per, n), e = min(b + per, n);
  i64 a = 0;
  for (i64 k = b; k < e; k += kPartBatch) {
    COUNT v[kPartBatch];
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) v[j] = k + j < e ? count[k + j] : (COUNT)0;
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) a += v[j];
  }
  sh[tid] = a;
  __syncthreads();
  for (int dd = 1; dd < kPartThreads; dd <<= 1) {
    const i64 o = tid >= dd ? sh[tid - dd] : 0;
    __syncthreads();
    sh[tid] += o;
    __syncthreads();
  }
  i64 run = tid > 0 ? sh[tid - 1] : 0;
  for (i64 k = b; k < e; k += kPartBatch) {
    COUNT v[kPartBatch];
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) v[j] = k + j < e ? count[k + j] : (COUNT)0;
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) if (k + j < e) { base[k + j] = run; run += v[j]; }
  }
  if (tid == kPartThreads - 1) base[n] = sh[tid];
  __syncthreads();
}

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// windows i and i + 1 of a vector (i even, the vector 16-byte aligned); what lies behind the end reads as 0
__device__ __forceinline__ u64x2 load_pair(const unsigned long long *__restrict__ p, long long i, long long n)
{
  if (i + 1 < n) return __builtin_nontemporal_load((const u64x2 *)(p + i));
  u64x2 v; v.x = i < n ? __builtin_nontemporal_load(p + i) : 0ull; v.y = 0ull;
  return v;
}

// what a rule need not say
struct CompactRule {
  static constexpr bool kTwoRowsInFlight = false;
  size_t lds_bytes() const { return 0; }
  __device__ __forceinline__ void block() {}
  __device__ __forceinline__ bool tile(long long, long long, int) { return true; }
};

// EMIT = false: the tile's number of kept windows.  EMIT = true: the kept windows' ordinals and rows at tileBase[tile] + rank.
template <class Rule, class Out, bool EMIT>
__global__ __launch_bounds__(kCompactThreads) void compact_kernel(Rule rule, long long n, unsigned *__restrict__ tileCount, const long long *__restrict__ tileBase,
                                                                  long long capacity, long long *__restrict__ ordinals, Out *__restrict__ out)
{
  typedef long long i64;
  typedef unsigned long long u64;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  rule.block();
  const i64 t = (i64)blockIdx.x * (kCompactThreads / 64) + w;
  const i64 tileStart = t * kCompactTile, tileEnd = min(tileStart + kCompactTile, n);
  if (tileStart >= n) return;
  i64 base = 0;
  if (EMIT) {
    base = tileBase[t];
    if (tileBase[t + 1] == base || base >= capacity) return;         // nothing kept here, or everything behind the caller's room
  }
  if (!rule.tile(tileStart, tileEnd, lane)) {
    if (!EMIT && lane == 0) tileCount[t] = 0;
    return;
  }
  unsigned before = 0;                                                // kept in the rows in front (wave-uniform)
  auto row = [&](int r, bool whole) {                                 // whole: every window of the row lies in front of n
    const i64 i = tileStart + (i64)r * 128 + 2 * lane;
    typename Rule::Payload p0, p1;
    rule.load(i, n, p0, p1);
    const bool keep0 = (whole || i < n) && rule.keep(i, p0), keep1 = (whole || i + 1 < n) && rule.keep(i + 1, p1);
    const u64 b0 = __ballot(keep0), b1 = __ballot(keep1);
    if (EMIT) {
      const u64 below = (1ull << lane) - 1;
      const i64 g0 = base + before + __popcll(b0 & below) + __popcll(b1 & below), g1 = g0 + (keep0 ? 1 : 0);
      if (keep0 && g0 < capacity) { ordinals[g0] = i; rule.emit(out, g0, i, p0); }
      if (keep1 && g1 < capacity) { ordinals[g1] = i + 1; rule.emit(out, g1, i + 1, p1); }
    }
    before += (unsigned)(__popcll(b0) + __popcll(b1));
  };
  if (Rule::kTwoRowsInFlight && tileEnd - tileStart == kCompactTile) {   // a whole tile: a fixed number of rows and no test between them
#pragma unroll 2
    for (int r = 0; r < kCompactRows; r++) row(r, true);
  } else {
#pragma unroll 2
    for (int r = 0; r < kCompactRows; r++) {
      if (tileStart + (i64)r * 128 >= tileEnd) break;                 // the first row behind n
      row(r, false);
    }
  }
  if (!EMIT && lane == 0) tileCount[t] = before;
}

// tileCount [tiles], tileBase [tiles + 1]: scratch.  ordinals int64 [capacity], out: the rule's rows, capacity of them.  n >= 1.  The
// number kept is tileBase[tiles] once the stream has run.
template <class Rule, class Out>
hipError_t launch_compact(const Rule &rule, long long n, unsigned *tileCount, long long *tileBase, long long capacity, long long *ordinals, Out *out, hipStream_t st)
{
  const long long nt = compact_tiles(n);
  const unsigned grid = (unsigned)((nt + kCompactThreads / 64 - 1) / (kCompactThreads / 64));
  const size_t lds = rule.lds_bytes();
  hipLaunchKernelGGL((compact_kernel<Rule, Out, false>), dim3(grid), dim3(kCompactThreads), lds, st, rule, n, tileCount, (const long long *)nullptr, capacity,
                     (long long *)nullptr, (Out *)nullptr);
  const hipError_t e = launch_tile_prefix(tileCount, nt, tileBase, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((compact_kernel<Rule, Out, true>), dim3(grid), dim3(kCompactThreads), lds, st, rule, n, (unsigned *)nullptr, tileBase, capacity, ordinals, out);
  return hipGetLastError();
}

}  // namespace gtx
