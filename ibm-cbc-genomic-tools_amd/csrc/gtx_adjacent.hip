// Kernels of the neighbour passes (see gtx_adjacent.h).  A tile is kAdjTile regions: four waves, each over a span of 8 rows of 64
// consecutive regions, lane l of a row reading region row * 64 + l -- the 12-bytes-per-lane non-temporal load pattern of link
// (gtx_link.hip).  The region in front of a lane's comes from the neighbouring lane (a wave shuffle), for lane 0 from the row in front,
// for the span's first region from one extra load; the gap pass takes the class of the region behind the same way.
#include <climits>
#include "gtx_adjacent.h"
#include "gtx_compact.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kWaves = kAdjThreads / 64;

// GenomicInterval::GetCoordinate (genomic_intervals.cpp:465-472): 5p / 3p by the interval's own strand
__device__ __forceinline__ i64 point_of(int s, int e, int minus, int op)
{
  return op == POINT_START ? s : op == POINT_STOP ? e : ((op == POINT_5P) != (minus != 0)) ? s : e;
}

// DIST: one int64 per region -- coord(i, op2) - coord(i - 1, op1) in the predecessor's class, LLONG_MIN otherwise and for region 0
template <bool DIST>
__global__ __launch_bounds__(kAdjThreads) void adjacent_pair_kernel(const int *__restrict__ tri, const unsigned char *__restrict__ minus, i64 n, int op1, int op2,
                                                                    i64 *__restrict__ dist, uint2 *__restrict__ tileSums, u64 *__restrict__ firstUnsorted)
{
  __shared__ uint2 shSums[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 spanBase = (i64)blockIdx.x * kAdjTile + (i64)w * kAdjSpan;
  const bool strands = DIST && minus != nullptr;
  int prevC = 0, prevS = 0, prevE = 0, prevM = 0;                     // the region in front of the span (wave-uniform)
  if (spanBase > 0 && spanBase < n) {
    prevC = tri[3 * (spanBase - 1)]; prevS = tri[3 * (spanBase - 1) + 1]; prevE = tri[3 * (spanBase - 1) + 2];
    if (strands) prevM = minus[spanBase - 1];
  }
  int c[kAdjRows], s[kAdjRows], e[kAdjRows], m[kAdjRows];
#pragma unroll
  for (int k = 0; k < kAdjRows; k++) {
    const i64 i = spanBase + 64 * k + lane;
    c[k] = 0; s[k] = 0; e[k] = INT_MIN; m[k] = 0;
    if (i < n) {
      c[k] = __builtin_nontemporal_load(tri + 3 * i); s[k] = __builtin_nontemporal_load(tri + 3 * i + 1); e[k] = __builtin_nontemporal_load(tri + 3 * i + 2);
      if (strands) m[k] = __builtin_nontemporal_load(minus + i);
    }
  }
  unsigned nIn = 0, nOv = 0;
  i64 unsortedAt = -1;
#pragma unroll
  for (int k = 0; k < kAdjRows; k++) {
    const i64 i = spanBase + 64 * k + lane;
    const bool valid = i < n;
    int pc = __shfl_up(c[k], 1), ps = __shfl_up(s[k], 1), pe = __shfl_up(e[k], 1), pm = strands ? __shfl_up(m[k], 1) : 0;
    const int lc = k ? __shfl(c[k ? k - 1 : 0], 63) : prevC, ls = k ? __shfl(s[k ? k - 1 : 0], 63) : prevS, le = k ? __shfl(e[k ? k - 1 : 0], 63) : prevE;
    const int lm = !strands ? 0 : k ? __shfl(m[k ? k - 1 : 0], 63) : prevM;
    if (lane == 0) { pc = lc; ps = ls; pe = le; pm = lm; }
    const bool pair = valid && i > 0, same = pair && c[k] == pc;
    const u64 ub = __ballot(pair && (c[k] < pc || (c[k] == pc && s[k] < ps)));
    if (ub && unsortedAt < 0) unsortedAt = spanBase + 64 * k + __builtin_ctzll(ub);
    const bool touch = same && s[k] <= pe;                            // RunGlobalTest :4765-4769
    nIn += (unsigned)__popcll(__ballot(touch && e[k] <= pe));
    nOv += (unsigned)__popcll(__ballot(touch && e[k] > pe));
    if (DIST && valid) {
      const i64 d = same ? point_of(s[k], e[k], m[k], op2) - point_of(ps, pe, pm, op1) : LLONG_MIN;
      __builtin_nontemporal_store(d, dist + i);
    }
  }
  if (lane == 0) {
    shSums[w] = make_uint2(nIn, nOv);
    if (unsortedAt >= 0) atomicMin(firstUnsorted, (u64)unsortedAt);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint2 t = shSums[0];
    for (int j = 1; j < kWaves; j++) { t.x += shSums[j].x; t.y += shSums[j].y; }
    tileSums[blockIdx.x] = t;
  }
}

// the tiles' sums added up in one block
__global__ __launch_bounds__(kPartThreads) void adjacent_reduce_kernel(const uint2 *__restrict__ tileSums, i64 nt, AdjInfo *info)
{
  __shared__ i64 shA[kPartThreads], shB[kPartThreads];
  const int tid = threadIdx.x;
  i64 a = 0, b = 0;
  for (i64 k = tid; k < nt; k += kPartThreads) { const uint2 v = tileSums[k]; a += v.x; b += v.y; }
  shA[tid] = a; shB[tid] = b;
  __syncthreads();
  for (int dd = kPartThreads / 2; dd > 0; dd >>= 1) {
    if (tid < dd) { shA[tid] += shA[tid + dd]; shB[tid] += shB[tid + dd]; }
    __syncthreads();
  }
  if (tid == 0) {
    info->nInclusions = shA[0]; info->nOverlaps = shB[0];
    info->firstUnsortedOut = info->firstUnsorted == ~0ull ? -1 : (i64)info->firstUnsorted;
  }
}

// ---- the gaps of RunGlobalInvert (:4576-4600) ----
// A region owns up to two gaps.  head = it opens a run (no region in front of it, or one of another class), tail = it closes one.
//   g0: head: [1, START - 1] when START > 1 (:4587); else [pSTOP + 1, START - 1] when START > pSTOP + 1, pSTOP its predecessor's (:4592)
//   g1: tail: [STOP + 1, size] when STOP + 1 < size (:4596), size the class's bound (none without a bound)
// STOP + 1 is taken in 64 bits; what is stored fits 32 (a bound is at most 2^31 - 3).
struct Gaps { bool g0, g1; int a0, b0, a1, b1; };
__device__ __forceinline__ i64 bound_of(const i64 *bounds, int nBounds, int c) { return c >= 0 && c < nBounds ? bounds[c] : -1; }
__device__ __forceinline__ Gaps gaps_of(bool head, bool tail, int c, int s, int e, int pe, const i64 *bounds, int nBounds)
{
  Gaps g;
  g.g0 = head ? s > 1 : (i64)s > (i64)pe + 1;
  g.a0 = head ? 1 : (int)((i64)pe + 1); g.b0 = (int)((i64)s - 1);
  const i64 size = tail ? bound_of(bounds, nBounds, c) : -1;
  g.g1 = size >= 0 && (i64)e + 1 < size;
  g.a1 = (int)((i64)e + 1); g.b1 = (int)size;
  return g;
}

// EMIT = false: the span's number of gaps, and the first bad region: one inside a run that starts before its predecessor, or the
// head of a run whose class has no bound.  EMIT = true: the gaps of the regions in front of the first bad one at spanBase[span] +
// rank, rank = the gaps of the rows in front (wave-uniform) plus the popcounts of the row's two ballots below the lane.
template <bool LDS, bool EMIT>
__global__ __launch_bounds__(kAdjThreads) void adjacent_gap_kernel(const int *__restrict__ tri, i64 n, const i64 *__restrict__ bounds, int nBounds,
                                                                   unsigned *__restrict__ spanCount, const i64 *__restrict__ spanBase, GapInfo *info, i64 capacity,
                                                                   unsigned *__restrict__ ownerOut, int *__restrict__ startOut, int *__restrict__ stopOut)
{
  extern __shared__ i64 shBounds[];
  if (LDS) {
    for (int j = threadIdx.x; j < nBounds; j += kAdjThreads) shBounds[j] = bounds[j];
    __syncthreads();
  }
  const i64 *B = LDS ? shBounds : bounds;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 span = (i64)blockIdx.x * kWaves + w, spanStart = span * kAdjSpan;
  if (spanStart >= n) { if (!EMIT && lane == 0) spanCount[span] = 0; return; }
  i64 base = 0;
  u64 limit = ~0ull;
  if (EMIT) {
    base = spanBase[span];
    limit = info->firstBad;
    if (spanBase[span + 1] == base || base >= capacity || (u64)spanStart >= limit) return;   // nothing here, no room, or behind the first bad region
  }
  int prevC = 0, prevS = 0, prevE = 0, nextC = 0;                     // the regions in front of and behind the span (wave-uniform)
  if (spanStart > 0) { prevC = tri[3 * (spanStart - 1)]; prevS = tri[3 * (spanStart - 1) + 1]; prevE = tri[3 * (spanStart - 1) + 2]; }
  if (spanStart + kAdjSpan < n) nextC = tri[3 * (spanStart + kAdjSpan)];
  int c[kAdjRows], s[kAdjRows], e[kAdjRows];
#pragma unroll
  for (int k = 0; k < kAdjRows; k++) {
    const i64 i = spanStart + 64 * k + lane;
    c[k] = 0; s[k] = 0; e[k] = INT_MIN;
    if (i < n) { c[k] = __builtin_nontemporal_load(tri + 3 * i); s[k] = __builtin_nontemporal_load(tri + 3 * i + 1); e[k] = __builtin_nontemporal_load(tri + 3 * i + 2); }
  }
  unsigned before = 0;                                                // gaps of the rows in front (wave-uniform)
  i64 badAt = -1;
#pragma unroll
  for (int k = 0; k < kAdjRows; k++) {
    const i64 i = spanStart + 64 * k + lane;
    const bool valid = i < n;
    int pc = __shfl_up(c[k], 1), ps = __shfl_up(s[k], 1), pe = __shfl_up(e[k], 1), nc = __shfl_down(c[k], 1);
    const int lc = k ? __shfl(c[k ? k - 1 : 0], 63) : prevC, ls = k ? __shfl(s[k ? k - 1 : 0], 63) : prevS, le = k ? __shfl(e[k ? k - 1 : 0], 63) : prevE;
    const int fc = k + 1 < kAdjRows ? __shfl(c[k + 1 < kAdjRows ? k + 1 : k], 0) : nextC;
    if (lane == 0) { pc = lc; ps = ls; pe = le; }
    if (lane == 63) nc = fc;
    const bool head = i == 0 || c[k] != pc, tail = i + 1 >= n || nc != c[k];
    Gaps g = gaps_of(head, tail, c[k], s[k], e[k], pe, B, nBounds);
    g.g0 &= valid; g.g1 &= valid;
    const u64 b0 = __ballot(g.g0), b1 = __ballot(g.g1);
    if (!EMIT) {
      const u64 bb = __ballot(valid && (head ? bound_of(B, nBounds, c[k]) < 0 : s[k] < ps));
      if (bb && badAt < 0) badAt = spanStart + 64 * k + __builtin_ctzll(bb);
    } else if ((u64)i < limit) {
      const u64 below = (1ull << lane) - 1;
      const i64 r0 = base + before + __popcll(b0 & below) + __popcll(b1 & below), r1 = r0 + (g.g0 ? 1 : 0);
      if (g.g0 && r0 < capacity) { ownerOut[r0] = (unsigned)i; startOut[r0] = g.a0; stopOut[r0] = g.b0; }
      if (g.g1 && r1 < capacity) { ownerOut[r1] = (unsigned)i; startOut[r1] = g.a1; stopOut[r1] = g.b1; }
    }
    before += (unsigned)(__popcll(b0) + __popcll(b1));
  }
  if (!EMIT && lane == 0) {
    spanCount[span] = before;
    if (badAt >= 0) atomicMin(&info->firstBad, (u64)badAt);
  }
}

// exclusive sum of the spans' counts in one block (block_exclusive_sum, gtx_compact.h); base[ns] = all gaps.  Then what is reported:
// without a bad region all of them, else the gaps owned by the regions in front of the first bad one, U -- those of the spans in
// front of U's and of the regions of U's span below U, counted here by one lane each.
__global__ __launch_bounds__(kPartThreads) void adjacent_prefix_kernel(const unsigned *__restrict__ count, i64 ns, i64 *__restrict__ base, const int *__restrict__ tri,
                                                                      i64 n, const i64 *__restrict__ bounds, int nBounds, GapInfo *info)
{
  __shared__ i64 sh[kPartThreads];
  const int tid = threadIdx.x;
  block_exclusive_sum(count, ns, base, sh);
  const u64 U = info->firstBad;
  const i64 spanOfU = U == ~0ull ? 0 : (i64)(U / kAdjSpan);
  i64 mine = 0;
  const i64 r = spanOfU * kAdjSpan + tid;
  if (U != ~0ull && (u64)r < U) {                                     // (r + 1 <= U < n: the region behind r exists)
    const int c = tri[3 * r], s = tri[3 * r + 1], e2 = tri[3 * r + 2];
    const bool head = r == 0 || tri[3 * (r - 1)] != c, tail = tri[3 * (r + 1)] != c;
    const Gaps g = gaps_of(head, tail, c, s, e2, r > 0 ? tri[3 * (r - 1) + 2] : 0, bounds, nBounds);
    mine = (g.g0 ? 1 : 0) + (g.g1 ? 1 : 0);
  }
  sh[tid] = mine;
  __syncthreads();
  for (int dd = kPartThreads / 2; dd > 0; dd >>= 1) {
    if (tid < dd) sh[tid] += sh[tid + dd];
    __syncthreads();
  }
  if (tid == 0) {
    if (U == ~0ull) { info->nGaps = base[ns]; info->firstBadOut = -1; info->badKind = 0; }
    else {
      info->nGaps = base[spanOfU] + sh[0]; info->firstBadOut = (i64)U;
      info->badKind = U == 0 || tri[3 * U] != tri[3 * (U - 1)] ? 2 : 1;
    }
  }
}

template <bool LDS>
void launch_gap_passes(const int *tri, i64 n, const i64 *bounds, int nBounds, i64 capacity, unsigned *spanCount, i64 *spanBase, GapInfo *info, unsigned *ownerOut,
                       int *startOut, int *stopOut, hipStream_t st)
{
  const i64 nt = adjacent_tiles(n), ns = adjacent_spans(n);
  const size_t lds = LDS ? (size_t)nBounds * sizeof(i64) : 0;
  hipLaunchKernelGGL((adjacent_gap_kernel<LDS, false>), dim3((unsigned)nt), dim3(kAdjThreads), lds, st, tri, n, bounds, nBounds, spanCount, (const i64 *)nullptr, info,
                     capacity, (unsigned *)nullptr, (int *)nullptr, (int *)nullptr);
  hipLaunchKernelGGL(adjacent_prefix_kernel, dim3(1), dim3(kPartThreads), 0, st, (const unsigned *)spanCount, ns, spanBase, tri, n, bounds, nBounds, info);
  hipLaunchKernelGGL((adjacent_gap_kernel<LDS, true>), dim3((unsigned)nt), dim3(kAdjThreads), lds, st, tri, n, bounds, nBounds, (unsigned *)nullptr,
                     (const i64 *)spanBase, info, capacity, ownerOut, startOut, stopOut);
}

}  // namespace

hipError_t launch_adjacent(const int *tri, const unsigned char *minus, long long n, int op1, int op2, long long *dist, uint2 *tileSums, AdjInfo *info, hipStream_t st)
{
  const i64 nt = adjacent_tiles(n);
  hipError_t e = hipMemsetAsync(info, 0xff, sizeof(u64), st);         // firstUnsorted = none
  if (e != hipSuccess) return e;
  if (dist) hipLaunchKernelGGL(adjacent_pair_kernel<true>, dim3((unsigned)nt), dim3(kAdjThreads), 0, st, tri, minus, n, op1, op2, dist, tileSums, &info->firstUnsorted);
  else hipLaunchKernelGGL(adjacent_pair_kernel<false>, dim3((unsigned)nt), dim3(kAdjThreads), 0, st, tri, minus, n, op1, op2, (i64 *)nullptr, tileSums, &info->firstUnsorted);
  hipLaunchKernelGGL(adjacent_reduce_kernel, dim3(1), dim3(kPartThreads), 0, st, (const uint2 *)tileSums, nt, info);
  return hipGetLastError();
}

hipError_t launch_gaps(const int *tri, long long n, const long long *bounds, int nBounds, long long capacity, unsigned *spanCount, long long *spanBase, GapInfo *info,
                       unsigned *ownerOut, int *startOut, int *stopOut, hipStream_t st)
{
  hipError_t e = hipMemsetAsync(info, 0xff, sizeof(u64), st);         // firstBad = none
  if (e != hipSuccess) return e;
  if (nBounds <= kAdjLdsBounds) launch_gap_passes<true>(tri, n, bounds, nBounds, capacity, spanCount, spanBase, info, ownerOut, startOut, stopOut, st);
  else launch_gap_passes<false>(tri, n, bounds, nBounds, capacity, spanCount, spanBase, info, ownerOut, startOut, stopOut, st);
  return hipGetLastError();
}

}  // namespace gtx
