// The annotate pass (gtx_join_annotate / gtx_pair_annotate_device, include/gtx.h): over the pairs of the overlap join (gtx_join.h)
// against a reference set whose first nPrimary ordinals are the genes and the rest their upstream regions, the per-pair rule of
// the reference's genomic_overlaps annotate (gtools/genomic_overlaps.cpp:268-290, :335-344): the offsets of the test region from
// the reference region (GetOffsetFrom, genomic_intervals.cpp:646-667; gtx_offset.h) with one op below nPrimary and another from
// there on, and under `center` only the pairs whose offset sum is not negative.  What is left in HBM is a CSR of the pairs that
// will be printed: kept offsets per query, and per kept pair its reference ordinal and its value (start + stop offset under
// center, the start offset otherwise -- the host halves, so the .5 of a centre stays exact).
//
// count per query -> exclusive scan (launch_join_scan) -> emit, over the segment walk of the offset pass: one lane per query;
// segments longer than kOffSmallSeg are listed by the count pass and taken by one block each in both passes.  Kept pairs stay in
// pair order: a lane writes its own in sequence, a block places each tile of 256 pairs behind the one before it.  Every
// dependency between blocks is a kernel boundary.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_offset.h"

namespace gtx {

enum : int { ANN_CENTER = 1, ANN_START = 2 };

struct AnnotateArgs {
  const int *tri;                // (class, start, stop) per query
  const int4 *refEnds;           // per reference ordinal: {front start, front stop, back start, back stop}
  const signed char *refStrand;  // '+' / '-' per reference ordinal (nullptr: '+')
  long long nRefs, nPrimary;     // ordinals < nPrimary take opPrimary, the others opRest; an ordinal outside [0, nRefs) is dropped
  int opPrimary, opRest;         // OFF_*
  int mode;                      // ANN_*
};

// cnt[t - q0] = the kept pairs of query t in [q0, q1) (off, pairs, nPairs as in launch_pair_offsets); big: q1 - q0 + 1 entries, the
// list of long segments, which launch_annotate_emit reads again
hipError_t launch_annotate_count(const AnnotateArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                                 long long *cnt, unsigned *big, hipStream_t st);
// the kept pairs of query t at keptRef / keptValue [koff[t - q0] ...] (koff: the exclusive scan of cnt), those below cap only
hipError_t launch_annotate_emit(const AnnotateArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                                const long long *koff, int *keptRef, long long *keptValue, long long cap, const unsigned *big, hipStream_t st);

}  // namespace gtx
