// Kernels of the window filter (see gtx_filter.h): the reference side, and the pass over the windows as a rule of the tile compaction
// (gtx_compact.h, which has the shape of the passes).
#include <limits.h>
#include "gtx_filter.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;

// ---- the reference side ----
// a region that takes part keeps its class, its start clamped to 1; any other goes into class nClasses, behind all of them
__global__ __launch_bounds__(256) void filter_prepare_kernel(const int *__restrict__ tri, i64 n, int nClasses, int *__restrict__ keyed, unsigned *__restrict__ bad)
{
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    const int c = tri[3 * i], s = tri[3 * i + 1], e = tri[3 * i + 2];
    const bool known = (unsigned)c < (unsigned)nClasses;
    if (!known) atomicOr(bad, 1u);
    const bool part = known && e >= 1 && s <= e;
    keyed[3 * i] = part ? c : nClasses; keyed[3 * i + 1] = s < 1 ? 1 : s; keyed[3 * i + 2] = e;
  }
}

// first[c] = the first sorted region of class c or of a later one, c = 0 .. nClasses + 1 (first[nClasses + 1] = n)
__global__ __launch_bounds__(256) void filter_first_kernel(const int *__restrict__ sorted, i64 n, int nClasses, int *__restrict__ first)
{
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    const int c = sorted[3 * i], p = i > 0 ? sorted[3 * (i - 1)] : -1;
    for (int k = p + 1; k <= c; k++) first[k] = (int)i;
    if (i == n - 1) for (int k = c + 1; k <= nClasses + 1; k++) first[k] = (int)n;
  }
}

// start[i], and runmax[i] = the largest stop among the sorted regions of i's class up to i: a segmented scan in one block, each thread
// over a run of consecutive regions, the runs' summaries joined by tile_exclusive (gtx_scan.h).  A run's summary is {a class begins
// inside it, the largest stop since the last such beginning}; summaries combine left to right.
constexpr int kRunThreads = 1024;
struct CutMax { int cut, m; };
struct CutMaxComb { __device__ __forceinline__ CutMax operator()(CutMax a, CutMax b) const { return CutMax{a.cut | b.cut, b.cut ? b.m : max(a.m, b.m)}; } };

__global__ __launch_bounds__(kRunThreads) void filter_runmax_kernel(const int *__restrict__ sorted, i64 n, int *__restrict__ start, int *__restrict__ runmax)
{
  __shared__ CutMax waveSum[kRunThreads / 64];
  const int tid = threadIdx.x;
  const i64 per = (n + kRunThreads - 1) / kRunThreads, b = min((i64)tid * per, n), e = min(b + per, n);
  int cut = 0, m = INT_MIN;
  int prev = b > 0 && b < n ? sorted[3 * (b - 1)] : -1;
#pragma unroll 4
  for (i64 i = b; i < e; i++) {
    const int c = sorted[3 * i], stop = sorted[3 * i + 2];
    if (c != prev) { cut = 1; m = stop; } else m = max(m, stop);
    prev = c;
  }
  int run = gtxscan::tile_exclusive<kRunThreads>(CutMax{cut, m}, waveSum, (CutMax *)nullptr, CutMax{0, INT_MIN}, CutMaxComb()).m;
  prev = b > 0 && b < n ? sorted[3 * (b - 1)] : -1;
#pragma unroll 4
  for (i64 i = b; i < e; i++) {
    const int c = sorted[3 * i], s = sorted[3 * i + 1], stop = sorted[3 * i + 2];
    run = c != prev ? stop : max(run, stop);
    prev = c;
    start[i] = s; runmax[i] = run;
  }
}

// ---- the pass over the windows ----
// lo + the number of arr[lo .. hi) that are <= key (arr ascending), found by the whole wave with 64 probes a step: every lane calls
// it with the same arguments and gets the same answer
__device__ __forceinline__ int wave_upper_bound(const int *__restrict__ arr, int lo, int hi, i64 key, int lane)
{
  while (hi > lo) {
    const i64 stride = ((i64)hi - lo + 63) >> 6, p = lo + lane * stride;
    const int c = __popcll(__ballot(p < hi && arr[p] <= key));       // the probes at or below the key are the first c
    if (c == 0) return lo;
    const i64 nhi = lo + c * stride;
    lo = (int)(lo + (c - 1) * stride + 1); hi = (int)min(nhi, (i64)hi);
  }
  return lo;
}

// the same for one lane
__device__ __forceinline__ int upper_bound(const int *__restrict__ arr, int lo, int hi, i64 key)
{
  while (hi > lo) {
    const int mid = lo + ((hi - lo) >> 1);
    if (arr[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// what a lane needs to test a window: the ordinals of the window's class, the class' first region, the range of the sorted regions
// the window's stop can fall into
struct Span { i64 off, end; int first, lo, hi; };

__device__ __forceinline__ bool overlaps(const FilterRefs &r, const Span &s, i64 i)
{
  if (i < s.off || i >= s.end) return false;
  const i64 a = (i64)r.step * (i - s.off) + 1, b = a + r.size - 1;
  const int j = upper_bound(r.start, s.lo, s.hi, b);
  return j > s.first && r.runmax[j - 1] >= a;
}

// a tile that meets several classes: the lane looks its window's class up (b0 .. b1 are the classes the tile meets)
__device__ __forceinline__ bool overlaps_any(const FilterRefs &r, int b0, int b1, i64 i)
{
  int b = b0;
  while (b < b1 && r.blkEnd[b] <= i) b++;
  if (b == b1) return false;
  const int c = r.blkCls[b];
  const Span s = {r.blkOff[b], r.blkEnd[b], r.first[c], r.first[c], r.first[c + 1]};
  return overlaps(r, s, i);
}

// A window is kept when its value reaches minValue and a region overlaps it; its row is the value.
struct FilterRule : CompactRule {
  FilterRefs r;
  const u64 *win;
  u64 minValue;
  // of the wave's tile (tile): the classes it meets, b0 .. b1 of the classes in offset order (disjoint, none empty); whether that is
  // one class, and then its span
  int b0, b1;
  bool one;
  Span s;
  typedef u64 Payload;

  // per class, the tile's first and last window together: does any region reach them?
  __device__ __forceinline__ bool tile(i64 tileStart, i64 tileEnd, int lane)
  {
    b0 = 0; b1 = r.nBlk;
    while (b0 < b1) { const int mid = b0 + ((b1 - b0) >> 1); if (r.blkEnd[mid] <= tileStart) b0 = mid + 1; else b1 = mid; }
    while (b1 < r.nBlk && r.blkOff[b1] < tileEnd) b1++;
    one = b1 == b0 + 1;
    bool reach = false;
    s = {0, 0, 0, 0, 0};
    for (int b = b0; b < b1; b++) {
      const i64 off = r.blkOff[b], end = r.blkEnd[b];
      const int c = r.blkCls[b], first = r.first[c];
      const i64 k0 = max(tileStart, off) - off, k1 = min(tileEnd, end) - 1 - off;
      const int hi = wave_upper_bound(r.start, first, r.first[c + 1], (i64)r.step * k1 + r.size, lane);
      if (hi == first || r.runmax[hi - 1] < (i64)r.step * k0 + 1) continue;
      reach = true;
      if (one) { s.off = off; s.end = end; s.first = first; s.hi = hi; s.lo = wave_upper_bound(r.start, first, hi, (i64)r.step * k0 + r.size, lane); }
    }
    return reach;
  }
  __device__ __forceinline__ void load(i64 i, i64 n, u64 &p0, u64 &p1) const { const u64x2 v = load_pair(win, i, n); p0 = v.x; p1 = v.y; }
  __device__ __forceinline__ bool keep(i64 i, const u64 &v) const { return v >= minValue && (one ? overlaps(r, s, i) : overlaps_any(r, b0, b1, i)); }
  __device__ __forceinline__ void emit(u64 *__restrict__ values, i64 g, i64, const u64 &v) const { values[g] = v; }
};

inline unsigned stride_grid(i64 n) { return (unsigned)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384); }

}  // namespace

hipError_t launch_filter_prepare(const int *tri, long long n, int nClasses, int *keyed, unsigned *bad, hipStream_t st)
{
  hipLaunchKernelGGL(filter_prepare_kernel, dim3(stride_grid(n)), dim3(256), 0, st, tri, n, nClasses, keyed, bad);
  return hipGetLastError();
}

hipError_t launch_filter_index(const int *sorted, long long n, int nClasses, int *first, int *start, int *runmax, hipStream_t st)
{
  hipLaunchKernelGGL(filter_first_kernel, dim3(stride_grid(n)), dim3(256), 0, st, sorted, n, nClasses, first);
  hipLaunchKernelGGL(filter_runmax_kernel, dim3(1), dim3(kRunThreads), 0, st, sorted, n, start, runmax);
  return hipGetLastError();
}

hipError_t launch_window_filter(const FilterRefs &r, const unsigned long long *windows, long long n, unsigned long long minValue, unsigned *tileCount,
                                long long *tileBase, long long capacity, long long *ordinals, unsigned long long *values, hipStream_t st)
{
  FilterRule rule = {};
  rule.r = r; rule.win = windows; rule.minValue = minValue;
  return launch_compact(rule, n, tileCount, tileBase, capacity, ordinals, values, st);
}

}  // namespace gtx
