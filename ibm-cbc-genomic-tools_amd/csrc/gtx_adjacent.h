// The neighbour passes (gtx_adjacent / gtx_gaps, include/gtx.h): what the reference's `genomic_regions test`, `gdist` and `inv`
// (RunGlobalTest genomic_intervals.cpp:4755-4778, RunGlobalCalcDistances :4523-4542, RunGlobalInvert :4576-4600) compute over a
// position-sorted region stream.  All three compare a region with the one directly in front of it (inv also with the one behind it),
// so nothing is carried along the stream: one streaming pass over the packed triples, 12 bytes per region.
//
//   adjacent_pair_kernel      per tile of kAdjTile regions: the first region before its predecessor in (class, start) (a 64-bit
//                             atomicMin), the tile's inclusions and overlaps among same-class neighbour pairs, and optionally one
//                             int64 distance per region
//   adjacent_reduce_kernel    the tiles' sums added up (one block)
//
//   adjacent_gap_kernel<.., false>   per span (one wave's kAdjSpan regions of a tile) the number of gaps its regions own -- a region
//                                    owns its leading or between gap, then its trailing gap -- and the first bad region
//   adjacent_prefix_kernel           exclusive sum of the spans' counts (one block); the gaps in front of the first bad region
//   adjacent_gap_kernel<.., true>    the gaps at span base + rank inside the span (ballots / popcounts), in stream order
//
// No block waits for another: every dependency between tiles is a kernel boundary.
#pragma once
#include <hip/hip_runtime.h>

namespace gtx {

constexpr int kAdjThreads = 256, kAdjRows = 8, kAdjTile = kAdjThreads * kAdjRows;   // (= GTX_ADJACENT_TILE)
constexpr int kAdjSpan = 64 * kAdjRows;                                             // regions per wave
constexpr int kAdjLdsBounds = 4096;                                                 // class bounds kept in LDS up to this many (32 KB)

enum : int { POINT_START = 0, POINT_STOP = 1, POINT_5P = 2, POINT_3P = 3 };

struct AdjInfo { unsigned long long firstUnsorted; long long nInclusions, nOverlaps, firstUnsortedOut; };   // firstUnsorted: ~0 = none
struct GapInfo { unsigned long long firstBad; long long nGaps, firstBadOut; int badKind, pad; };            // firstBad: ~0 = none

inline long long adjacent_tiles(long long n) { return (n + kAdjTile - 1) / kAdjTile; }
inline long long adjacent_spans(long long n) { return adjacent_tiles(n) * (kAdjTile / kAdjSpan); }

// tri: n >= 1 (class, start, stop) triples in stream order; minus: one strand byte per region or NULL (all '+'); dist: n int64 or NULL.
// tileSums holds adjacent_tiles(n) entries.
hipError_t launch_adjacent(const int *tri, const unsigned char *minus, long long n, int op1, int op2, long long *dist, uint2 *tileSums, AdjInfo *info,
                           hipStream_t st);

// bounds: nBounds int64 (missing: < 0).  spanCount holds adjacent_spans(n) entries, spanBase one more.  The outputs hold `capacity`
// gaps; a gap whose rank is >= capacity is not written.
hipError_t launch_gaps(const int *tri, long long n, const long long *bounds, int nBounds, long long capacity, unsigned *spanCount, long long *spanBase,
                       GapInfo *info, unsigned *ownerOut, int *startOut, int *stopOut, hipStream_t st);

}  // namespace gtx
