// Link (gtx_link / gtx_link_device, include/gtx.h): a position-sorted region stream merged into its covered territory -- the
// reference's `genomic_regions link` (RunGlobalLink, genomic_intervals.cpp:4605-4644).  The sequential loop keeps a running maximum
// of the open group's stops; its group boundaries, though, are those of a class-segmented prefix maximum over ALL stops in front of a
// region (proof in gtx.h), so the work is three streaming passes over the packed triples and two one-block scans of per-tile values:
//
//   link_scan_kernel<false>   per tile of kLinkTile regions the (class break seen, maximum stop since) aggregate; the order check
//   link_prefix_kernel        exclusive scan of the tile aggregates (one block)
//   link_scan_kernel<true>    the same tile scan seeded with the tile's prefix: one break flag per region, as a bit map (a wave's
//                             ballot is 64 consecutive regions), and the heads of each tile
//   link_heads_kernel         exclusive sum of the tiles' heads (one block); the group count in front of the first unsorted region
//   link_init_kernel          the identity into the records of groups that continue over a tile boundary
//   link_groups_kernel        per group its head, member count, maximum stop and folded value: groups inside a tile are stored, the
//                             pieces of a group that crosses tiles are combined with integer atomics (commutative: the result does
//                             not depend on the order the tiles run in)
//
// No block waits for another: every dependency between tiles is a kernel boundary.
#pragma once
#include <hip/hip_runtime.h>

namespace gtx {

constexpr int kLinkThreads = 256, kLinkRows = 8, kLinkTile = kLinkThreads * kLinkRows;   // (= GTX_LINK_TILE)

enum : int { LINK_NONE = 0, LINK_SUM = 1, LINK_MIN = 2, LINK_MAX = 3 };

struct LinkInfo { unsigned long long firstUnsorted; long long nGroups, firstUnsortedOut; };   // firstUnsorted: ~0 = none

// scratch of one call, sized by link_tiles(n): tileAgg, tilePrefix [tiles] int2; bits [tiles * kLinkTile / 64]; tileHeads [tiles];
// tileHeadBase [tiles + 1]; info [1]
struct LinkWork {
  int2 *tileAgg, *tilePrefix;
  unsigned long long *bits;
  unsigned *tileHeads;
  long long *tileHeadBase;
  LinkInfo *info;
};

inline long long link_tiles(long long n) { return (n + kLinkTile - 1) / kLinkTile; }

// tri: n (class, start, stop) triples in stream order; vals: one int64 per region (mode != LINK_NONE).  Outputs hold n entries; the
// first info->nGroups are written.  n >= 1.
hipError_t launch_link(const int *tri, const long long *vals, long long n, long long maxDifference, int mode, const LinkWork &w,
                       unsigned *headOut, unsigned *countOut, int *stopOut, long long *valOut, hipStream_t st);


// The tool's text path: the triples the tokenizer made of a plain block (class = chromosome id, + nChrom on the '-' strand) appended
// to the link input as link classes (the id, or 2 * id + strand when the set is sorted by strand) with the strand kept beside them;
// *bad is raised when a line has no class (a chromosome the table lacks).
hipError_t launch_link_append(const int *src, long long n, int nChrom, int byStrand, int *dst, unsigned char *minus, int *bad, hipStream_t st);
// per reported group {2 * chromosome id + strand, start} of its head
hipError_t launch_link_head_keys(const int *tri, const unsigned char *minus, const unsigned *head, const LinkInfo *info, long long n, int byStrand, int2 *out,
                                 hipStream_t st);

}  // namespace gtx
