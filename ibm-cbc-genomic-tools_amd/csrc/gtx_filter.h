// Window filter (gtx_window_refs / gtx_window_filter / gtx_window_filter_device, include/gtx.h): which windows of a scan overlap a
// reference region and hold at least min_value -- the -r filter of `genomic_scans counts`, GenomicRegionSetIndex::GetOverlap(&w, false,
// ignore_strand) of the reference (genomic_intervals.cpp:5489-5540) for single-interval regions, asked once per window there.  Window k
// of a class with step D and size W is [D k + 1, D k + W]; a region [s, e] takes part when e >= 1 and s <= e, its start clamped to 1.
//
// The reference side, once per region set (launch_filter_prepare, then the device sort, then launch_filter_index):
//
//   filter_prepare_kernel      a region that takes no part goes into one class behind all others: the sort leaves it at the end
//   gtx_sort_device            (class, start) order
//   filter_first_kernel        per class the first region of the sorted order
//   filter_runmax_kernel       the starts, and the class-segmented running maximum of the stops (one block, the shape of the tile prefix)
//
// A window [a, b] of class c overlaps a region exactly when j = upper_bound(start of c, b) lies behind first[c] and runmax[j - 1] >= a.
//
// The pass over the windows is a rule of the tile compaction (gtx_compact.h): a kept window comes out with its ordinal and its value.
// A tile first asks for its first and last window together (two searches the whole wave makes, 64 probes a step); when no region
// reaches it, it is done without loading a window.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_compact.h"

namespace gtx {

constexpr int kFilterTile = kCompactTile;                            // (include/gtx.h names it: GTX_FILTER_TILE)

// the prepared region set and the layout of the window vector it was prepared for
struct FilterRefs {
  const int *start, *runmax;                                         // [nRefs], (class, start) order; the regions that take no part at the end
  const int *first;                                                  // [nClasses + 1]: a class' regions are first[c] .. first[c + 1]
  const long long *blkOff, *blkEnd;                                  // [nBlk] the classes that have windows, by offset: their ordinals blkOff[b] .. blkEnd[b]
  const int *blkCls;                                                 // [nBlk]
  int nBlk, step, size;
};

// tri [n x 3] -> keyed [n x 3] for the sort with nClasses + 1 classes; *bad != 0 afterwards: a class id outside [0, nClasses)
hipError_t launch_filter_prepare(const int *tri, long long n, int nClasses, int *keyed, unsigned *bad, hipStream_t st);
// sorted [n x 3] (the sort's output) -> first [nClasses + 2], start [n], runmax [n].  n >= 1
hipError_t launch_filter_index(const int *sorted, long long n, int nClasses, int *first, int *start, int *runmax, hipStream_t st);
// tileCount [tiles], tileBase [tiles + 1]: scratch, tiles = compact_tiles(n).  ordinals int64 [capacity], values uint64 [capacity].  n >= 1.  The number kept is
// tileBase[tiles] once the stream has run.
hipError_t launch_window_filter(const FilterRefs &r, const unsigned long long *windows, long long n, unsigned long long minValue, unsigned *tileCount,
                                long long *tileBase, long long capacity, long long *ordinals, unsigned long long *values, hipStream_t st);

}  // namespace gtx
