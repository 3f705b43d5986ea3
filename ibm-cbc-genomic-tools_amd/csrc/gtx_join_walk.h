// The walk of the overlap join (gtx_join.hip) over the envelope index, shared by every kernel that visits a query's pairs
// without writing them out first (gtx_signal.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_join.h"

namespace gtx {

// as in gtx_pairs.hip: does [s, e] overlap an interval of iv[0..n) (starts and stops non-decreasing)?
__device__ __forceinline__ bool overlaps_list(const int2 *__restrict__ iv, int n, int s, int e)
{
  int a = 0, b = n;
  while (a < b) { const int m = (a + b) >> 1; if (iv[m].y >= s) b = m; else a = m + 1; }
  return a < n && iv[a].x <= e;
}

struct Query { int cls, s, e; int2 blk; bool match; };

// which queries take part (the count path's rules, include/gtx.h GTX_ZERO_LENGTH_OK): an unknown class never; start > stop + 1
// only under merge semantics with GTX_ZERO_LENGTH_OK; start == stop + 1 with GTX_ZERO_LENGTH_OK
__device__ __forceinline__ Query load_query(const JoinQueries &q, long long t, const PairIndex &ix, int mode, bool &noClass, bool &degenerate)
{
  Query r;
  r.cls = q.tri[3 * t]; r.s = q.tri[3 * t + 1]; r.e = q.tri[3 * t + 2];
  r.blk = q.blk ? q.blk[t] : make_int2(0, 1);
  noClass = r.cls < 0 || r.cls >= ix.nClasses;
  const bool zeroOk = mode & JOIN_ZERO_OK;
  degenerate = !noClass && r.s > r.e + (zeroOk ? 1 : 0);
  r.match = !noClass && (!degenerate || (zeroOk && (mode & JOIN_MERGE)));
  return r;
}

// every region of ix the query overlaps, in descending order of envelope start (ties: descending ordinal); f(ordinal)
template <class F>
__device__ __forceinline__ void walk(const Query &q, const int2 *__restrict__ qIv, const PairIndex &ix, const RegionBlocks &rb, int mode, F &&f)
{
  const int lo = ix.seg[q.cls], hi = ix.seg[q.cls + 1];
  int a = lo, b = hi;
  while (a < b) { const int m = (a + b) >> 1; if (ix.start[m] <= q.e) a = m + 1; else b = m; }   // entries [lo, a) start at or before q.e
  const bool zeroOk = mode & JOIN_ZERO_OK, gaps = mode & JOIN_GAPS;
  const bool multiQ = !gaps && q.blk.y > 1;
  for (int i = a - 1; i >= lo;) {
    if (ix.pmax[i] < q.s) break;                                                                   // nothing further down reaches the query
    if ((i & 63) == 63 && i - 63 >= lo && ix.bmax[i >> 6] < q.s) { i -= 64; continue; }
    const int e = ix.end[i];
    if (e >= q.s) {
      const int s = ix.start[i];
      if (zeroOk || s <= e + 1) {                                                                  // an inverted region (merge set) only with GTX_ZERO_LENGTH_OK
        const int r = ix.id[i];
        bool hit = true;
        if (!gaps && (multiQ || rb.blkOf)) {
          const int2 blk = rb.blkOf ? rb.blkOf[r] : make_int2(0, 0);
          if (multiQ) {
            hit = false;
            for (int k = 0; k < q.blk.y && !hit; k++) {
              const int2 qi = qIv[q.blk.x + k];
              hit = blk.y ? overlaps_list(rb.iv + blk.x, blk.y, qi.x, qi.y) : (s <= qi.y && e >= qi.x);
            }
          } else if (blk.y) hit = overlaps_list(rb.iv + blk.x, blk.y, q.s, q.e);
        }
        if (hit) f(r);
      }
    }
    i--;
  }
}

}  // namespace gtx
