// Window selection (gtx_window_select / gtx_window_select_device, include/gtx.h): which windows of up to four scans are kept by a
// table rule, and their clamped counts -- the data pass of the reference's `genomic_apps peakdiff` (ScanReadFiles,
// genomic_apps.cpp:385-412) with its binomial tail folded into tables of critical counts (gtx_peakdiff.h).  With W the window size,
// k_f = min(v_f, W) the clamped sum of tested vector f and c_f = min(ctl_f, W) that of its control, a window is kept when
// k_f >= kcrit_f[c_f] for any f (kcrit_f[0] when there are no controls).  The kept windows come out in window order, each with its
// ordinal and one row of clamped counts (tested vectors, then controls): a rule of the tile compaction, gtx_compact.h.
//
// The tables are copied into LDS while they fit kSelectLdsBytes, and are read from global memory (L2) beyond that.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_compact.h"

namespace gtx {

constexpr int kSelectTile = kCompactTile;                            // (gtx_window_select_limits reports it)
constexpr int kSelectMaxTested = 4;
constexpr int kSelectLdsBytes = 64 * 1024;                           // tables of nTested * (W + 1) * 4 bytes up to this sit in LDS
constexpr int kSelectLdsMaxW = kSelectLdsBytes / (4 * kSelectMaxTested) - 1;   // ... i.e. with four tested vectors and controls, W up to this

struct SelectArgs {
  const unsigned long long *tested[kSelectMaxTested];                 // 16-byte aligned, n windows each
  const unsigned long long *control[kSelectMaxTested];                // all set or all null
  const int *tab;                                                    // table f at f * (W + 1) with controls, at f without
  int nTested, W;
  long long n;
};

inline bool select_tables_in_lds(int nTested, int W, bool controls) { return (long long)nTested * (controls ? W + 1 : 1) * 4 <= kSelectLdsBytes; }

// tileCount [tiles], tileBase [tiles + 1]: scratch, tiles = compact_tiles(n).  ordinals [capacity] int64, rows [capacity * (controls ? 2 : 1) * nTested]
// int32.  n >= 1.  The number kept is tileBase[tiles] once the stream has run.
hipError_t launch_window_select(const SelectArgs &a, unsigned *tileCount, long long *tileBase, long long capacity, long long *ordinals, int *rows,
                                hipStream_t st);

}  // namespace gtx
