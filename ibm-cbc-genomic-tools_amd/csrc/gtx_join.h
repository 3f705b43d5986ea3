// The overlap join (gtx_join / gtx_join_device, include/gtx.h): for a batch of queries in HBM, the reference ordinal of every
// (query, reference region) pair that overlaps, as a CSR array -- offsets per query, the pairs of a query in the order of a
// per-region key (the reference's iteration order: ascending ordinal for the sorted merge, (level, bin, -ordinal) for the bin
// index).  Three passes: count (one walk per query), an exclusive scan of the counts into 64-bit offsets, emit (the same walk,
// writing), then a sort of the segments whose walk order is not key order.
//
// Candidates come from the envelope index of gtx_pairs.h over all regions (PairIndex: per class the envelopes in the order of
// their starts, the running maximum of their ends, the per-64 maximum): a binary search for the last start <= the query's stop,
// then a walk down that ends where the running maximum falls below the query's start.  The pair test is the sorted merge's
// (CalcDirection == 0 on the envelopes, genomic_intervals.cpp:1225-1236), then, unless -gaps, some pair of intervals
// (GenomicRegion::OverlapsWith, :1167-1172).  Count and emit run the same walk, so a query's segment is exactly as long as
// its count.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_pairs.h"

namespace gtx {

struct JoinQueries {
  const int *tri;        // (class, start, stop) per query; the envelope of a multi-interval query
  const int2 *blk;       // {first, count} into iv per query; nullptr: every query has one interval
  const int2 *iv;        // {start, stop}, starts and stops non-decreasing within a query
  long long n;
};

enum : int {
  JOIN_ZERO_OK = 1,      // GTX_ZERO_LENGTH_OK: zero-length queries match; inverted ones (and inverted regions) too on a merge set
  JOIN_MERGE = 2,        // the reference set was given with GTX_REFS_KEEP_ZERO_LENGTH
  JOIN_CHECK = 4,        // GTX_CHECK_SORTED: first query whose (class, start) sorts before its predecessor's
  JOIN_GAPS = 8          // envelopes decide (-gaps): no interval test
};

// what the count pass observed (indices within the batch; INT64_MAX: none)
struct JoinInfo { long long noClass, degenerate, firstDegenerate, firstUnsorted, mismatch; };

// off[i] = number of pairs of query i (i < q.n); info accumulates
hipError_t launch_join_count(const JoinQueries &q, const PairIndex &ix, const RegionBlocks &rb, int mode, long long *off, JoinInfo *info, hipStream_t st);
// exclusive prefix sum of v[0..n) in place; partial: join_scan_partials(n) entries of scratch
long long join_scan_partials(long long n);
hipError_t launch_join_scan(long long *v, long long n, long long *partial, hipStream_t st);
// *cut = the largest q1 in [q0, n] with off[q1] - off[q0] <= cap (off: n + 1 offsets)
hipError_t launch_join_cut(const long long *off, long long q0, long long n, long long cap, long long *cut, hipStream_t st);
// pairs of queries [q0, q1) at pairs[off[i] - off[q0] ...], in ascending envelope start (ties: index order); a query whose walk
// does not find exactly its count bumps info->mismatch and writes no more than its count
hipError_t launch_join_emit(const JoinQueries &q, long long q0, long long q1, const PairIndex &ix, const RegionBlocks &rb, int mode,
                            const long long *off, int *pairs, JoinInfo *info, hipStream_t st);
// the segments of queries [q0, q1) into ascending (key[r], r) (key == nullptr: r).  Up to kJoinSmallSeg pairs: one lane each,
// in place; longer ones: one block each (bitonic sort in LDS up to kJoinLdsSeg pairs, above that sorted runs of kJoinLdsSeg
// merged pass by pass through scratch, which has the layout of pairs).  big: q1 - q0 + 1 entries of scratch (a list and its length).
constexpr int kJoinSmallSeg = 32;
constexpr int kJoinLdsSeg = 2048;
hipError_t launch_join_sort(const long long *off, long long q0, long long q1, const long long *key, int *pairs, int *scratch,
                            unsigned *big, hipStream_t st);

}  // namespace gtx
