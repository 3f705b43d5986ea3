// Pair offsets (gtx_join_offsets / gtx_pair_offsets_device, include/gtx.h): for the pairs of the overlap join (gtx_join.h), the
// reference's genomic_overlaps offset values (gtools/genomic_overlaps.cpp:545-670).  One side of a pair is the reference point
// (its front or back interval by op and strand: GenomicInterval::GetOffsetFrom, genomic_intervals.cpp:646-667), the other the
// region whose offsets are taken (its envelope).  Normally the point is the join's reference region and the offsets are the
// query's; with `fromQuery` the roles swap -- the sorted offset branch, where the merge's queries are the reference file.
//
// With skip-ref-gaps (CalcOffsetsWithoutGaps, :6154-6205) a pair has a variable number of entries: one per (reference interval k,
// query interval contained in it), in that loop order, each the query interval's offsets minus the gaps of the reference before
// (or after) interval k.  A pair whose query or reference intervals are not sorted and disjoint has none (the reference's
// warning case).  So that path runs count -> scan (launch_join_scan) -> emit.
//
// Every pass walks the CSR of the join (offsets per query, pairs) with one lane per query over its segment; segments longer than
// kOffSmallSeg are listed and taken by one block each, as launch_join_sort does.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_join.h"

namespace gtx {

enum : int { OFF_1 = 1, OFF_2 = 2, OFF_5P = 3, OFF_3P = 4 };

struct OffsetArgs {
  JoinQueries q;                 // the join's queries; blk / iv: their intervals (nullptr: one interval each)
  const signed char *qStrand;    // '+' / '-' per query (fromQuery only; nullptr: '+')
  const int4 *refEnds;           // per reference ordinal: {front start, front stop, back start, back stop}
  const signed char *refStrand;  // '+' / '-' per reference ordinal (nullptr: '+')
  RegionBlocks rb;               // the reference intervals (skip-ref-gaps); count 0: the region is its front interval
  int op;                        // OFF_*
  bool fromQuery;                // the query is the reference point, the reference region's envelope is offset
};

constexpr int kOffSmallSeg = 32;

// the reference point of a pair: front and back interval of a region and its strand
struct Point { int2 front, back; bool minus; };

// GenomicInterval::GetOffsetFrom(GenomicRegion *) of the interval [s, e] (genomic_intervals.cpp:646-667, GetCoordinate :465-472):
// the strand of the point decides both the interval (front / back) and the direction (within a pair the two strands agree
// unless -i, and under -i the reference's strand is the one used)
__device__ __forceinline__ void offset_from(const Point &pt, int op, long long s, long long e, long long &a, long long &b)
{
  const bool back = op == OFF_2 || (pt.minus && op == OFF_5P) || (!pt.minus && op == OFF_3P);
  const int2 iv = back ? pt.back : pt.front;
  const long long ref = op == OFF_1 ? iv.x : op == OFF_2 ? iv.y : op == OFF_5P ? (pt.minus ? iv.y : iv.x) : (pt.minus ? iv.x : iv.y);
  if ((pt.minus && op == OFF_5P) || (!pt.minus && op == OFF_3P)) { a = ref - e; b = ref - s; }
  else { a = s - ref; b = e - ref; }
}

// the pairs of queries [q0, q1): out[2 p], out[2 p + 1] = {start offset, stop offset} of pair p (p relative to off[q0]);
// *firstInverted = min over the pairs p < nPairs with start > stop (leave it at INT64_MAX beforehand).  big: q1 - q0 + 1 entries.
hipError_t launch_pair_offsets(const OffsetArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                               long long *out, long long *firstInverted, unsigned *big, hipStream_t st);
// skip-ref-gaps, count: cnt[p] = the number of entries of pair p
hipError_t launch_pair_gaps_count(const OffsetArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                                  long long *cnt, unsigned *big, hipStream_t st);
// skip-ref-gaps, emit: the entries of pair p at out[2 eoff[p] ...] (eoff: the exclusive scan of cnt)
hipError_t launch_pair_gaps_emit(const OffsetArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                                 const long long *eoff, long long *out, unsigned *big, hipStream_t st);
// refEnds from the envelopes ({start, stop} per ordinal) and the intervals of rb
hipError_t launch_ref_ends(const int2 *env, const RegionBlocks &rb, long long m, int4 *refEnds, hipStream_t st);

}  // namespace gtx
