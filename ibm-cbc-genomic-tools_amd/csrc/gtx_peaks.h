// Peak candidate selection (gtx_peak_select / gtx_peak_select_device, include/gtx.h): which windows of a signal scan `genomic_scans
// peaks` tests at all, and the three counts its tail probabilities are computed from -- the head of the reference's per-window loop
// (PeakFinder, genomic_scans.cpp:304-311).  With S, C and U the window sums of the signal, the control and the mappability track read
// as signed 64-bit values and W the window size:
//
//   v0 = U ? U[w] : W;   v1 = min(S[w], v0);   v2 = min(C[w], v0)
//   norm:  ratio < 1.0 ?  v2 = (long)floor((float)v2 * ratio)  :  v1 = (long)floor((float)v1 / ratio)
//   kept when v1 >= min_reads
//
// The conversion to float is the reference's (a count rounds to 24 bits before it is scaled); the product and the quotient are in
// double.  This file is compiled with -ffp-contract=off: the floor decides an integer, nothing may be fused around it.
//
// The kept windows come out in window order, each with its ordinal and the row v1, v2, v0: a rule of the tile compaction
// (gtx_compact.h).  Per window 16 bytes are read (24 with U) by each of the two passes that load it, 32 bytes are written per kept
// window.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_compact.h"

namespace gtx {

constexpr int kPeakTile = kCompactTile;                              // (include/gtx.h names it: GTX_PEAK_TILE)

struct PeakArgs {
  const unsigned long long *signal, *control, *uniq;                 // 16-byte aligned, n windows each; uniq may be null
  long long n, winSize, minReads;
  int norm;                                                          // 0: as counted, 1: the control scaled (ratio < 1), 2: the signal scaled
  double ratio;
};

// tileCount [tiles], tileBase [tiles + 1]: scratch, tiles = compact_tiles(n).  ordinals [capacity] int64, rows [capacity * 3] int64.  n >= 1.  The number kept
// is tileBase[tiles] once the stream has run.
hipError_t launch_peak_select(const PeakArgs &a, unsigned *tileCount, long long *tileBase, long long capacity, long long *ordinals, long long *rows,
                              hipStream_t st);

}  // namespace gtx
