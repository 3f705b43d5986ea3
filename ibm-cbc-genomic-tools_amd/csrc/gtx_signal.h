// Signal binned around reference points (gtx_signal_bins / gtx_signal_bins_device, include/gtx.h): the inner loop of the
// reference's genomic_apps profile and heatmap (gtools/genomic_apps.cpp:560-605, :826-880) fused into one pass.  One lane per
// read walks the envelope index as the join's count pass does (gtx_join_walk.h: the same pairs), takes for every pair the 5'
// offset of the read's front interval from the reference region (offset_from of gtx_offset.h, GetOffsetFrom
// genomic_intervals.cpp:646-667), and forms in double, in the reference's order of operations,
//     x = (double)(start + stop) / 2 / ref_len + bin_min,   z = (x - bin_min) / (bin_max - bin_min),   bin = (int)(n_bins * z)
// for 0 <= z < 1.  The pairs are never written out.  The file is compiled with -ffp-contract=off: a fused multiply-add would
// move reads across bin edges.
//
// Accumulation is exact: every read brings an int64 weight and the bins are int64 sums (64-bit atomics, wrap-around).  While
// the weights are integers and the partial sums stay below 2^53 in magnitude, (double) of a bin equals the reference's
// sequential double sum bit for bit, whatever order the atomics landed in.
//
// Two layouts: one shared row of n_bins (profile) -- a block keeps its own histogram in LDS while n_bins <= kSignalLdsBins and
// adds its non-zero bins to the row at the end; above that bound every pair adds to the row in HBM --, or one row per reference
// ordinal (heatmap, n_refs x n_bins), where every pair adds to its (row, bin) in HBM.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_join.h"

namespace gtx {

constexpr int kSignalLdsBins = 4096;     // 32 KB of LDS per block: five blocks (20 waves) still fit a CU

struct SignalArgs {
  JoinQueries q;                 // the reads; blk / iv: their intervals (nullptr: one each).  The offset is the front interval's
  const long long *w;            // weight per read (nullptr: 1)
  PairIndex ix; RegionBlocks rb; int mode;     // the join's index and rules (gtx_join.h JOIN_*)
  const int4 *refEnds;           // per reference ordinal: {front start, front stop, back start, back stop} (launch_ref_ends)
  const signed char *refStrand;  // '+' / '-' per reference ordinal (nullptr: '+')
  const long long *refLen;       // per reference ordinal, a size_t (nullptr: 1)
  double binMin, binMax;
  long long nBins;               // < 2^31
  bool perRef;                   // heatmap: row = reference ordinal
};

// what a call observed, summed over its reads
struct SignalInfo {
  unsigned long long pairs;      // pairs walked
  unsigned long long binned;     // pairs that landed in a bin
  unsigned long long dropped;    // 0 <= z < 1 but (int)(n_bins * z) == n_bins (rounding): the reference writes past its array
  unsigned long long absWeight;  // sum of |w| over the binned pairs
  unsigned long long noClass, degenerate;
  long long firstInverted;       // first read with a pair whose start offset exceeds its stop offset (INT64_MAX: none)
};

// bins[(perRef ? r * nBins : 0) + bin] += w over the pairs of reads [0, q.n); info accumulates (set it up beforehand: zeros,
// firstInverted INT64_MAX).  nCU: the device's compute units (the grid is the blocks they hold at once).
hipError_t launch_signal_bins(const SignalArgs &a, unsigned long long *bins, SignalInfo *info, int nCU, hipStream_t st);

}  // namespace gtx
