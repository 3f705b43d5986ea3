// Kernels of the pair offsets (see gtx_offset.h).
#include <climits>
#include "gtx_offset.h"

namespace gtx {
namespace {

__device__ __forceinline__ Point ref_point(const OffsetArgs &a, int r)
{
  const int4 v = a.refEnds[r];
  return Point{make_int2(v.x, v.y), make_int2(v.z, v.w), a.refStrand != nullptr && a.refStrand[r] == '-'};
}

__device__ __forceinline__ Point query_point(const OffsetArgs &a, long long t)
{
  Point p;
  if (a.q.blk) { const int2 b = a.q.blk[t]; p.front = a.q.iv[b.x]; p.back = a.q.iv[b.x + b.y - 1]; }
  else { p.front = make_int2(a.q.tri[3 * t + 1], a.q.tri[3 * t + 2]); p.back = p.front; }
  p.minus = a.qStrand != nullptr && a.qStrand[t] == '-';
  return p;
}

// IsCompatibleSortedAndNonoverlapping (:1139-1161) of an interval list: starts non-decreasing, each start after the last stop
template <class IV>
__device__ __forceinline__ bool sorted_disjoint(IV iv, int n)
{
  for (int k = 1; k < n; k++) { const int2 x = iv(k), y = iv(k - 1); if (x.x < y.x || x.x <= y.y) return false; }
  return true;
}

// CalcOffsetsWithoutGaps (:6176-6195) of one pair: entries in loop order (reference interval outer, query interval inner);
// with out == nullptr only counts them
__device__ __forceinline__ long long gaps_walk(const OffsetArgs &a, long long t, int r, long long *out)
{
  const int2 rblk = a.rb.blkOf ? a.rb.blkOf[r] : make_int2(0, 0);
  const int4 ends = a.refEnds[r];
  const int K = rblk.y ? rblk.y : 1;
  auto riv = [&](int k) { return rblk.y ? a.rb.iv[rblk.x + k] : make_int2(ends.x, ends.y); };
  const int2 qblk = a.q.blk ? a.q.blk[t] : make_int2(0, 1);
  const int2 qenv = make_int2(a.q.tri[3 * t + 1], a.q.tri[3 * t + 2]);
  auto qiv = [&](int j) { return a.q.blk ? a.q.iv[qblk.x + j] : qenv; };
  const int J = qblk.y;
  if (!sorted_disjoint(qiv, J) || !sorted_disjoint(riv, K)) return 0;
  const Point pt = ref_point(a, r);
  // GetGapSizes (:6154-6172): forward sums for 1, +5p, -3p, backward otherwise; backward gap[k] = total - forward gap[k]
  const bool forward = a.op == OFF_1 || (!pt.minus && a.op == OFF_5P) || (pt.minus && a.op == OFF_3P);
  long long total = 0;
  for (int k = 1; k < K; k++) total += (long long)riv(k).x - riv(k - 1).y - 1;
  long long fwd = 0, n = 0;
  for (int k = 0; k < K; k++) {
    const int2 rk = riv(k);
    if (k > 0) fwd += (long long)rk.x - riv(k - 1).y - 1;
    const long long gap = forward ? fwd : total - fwd;
    for (int j = 0; j < J; j++) {
      const int2 qj = qiv(j);
      if (qj.x >= rk.x && qj.y <= rk.y) {                                   // IsContained (:613-618)
        if (out) { long long s, e; offset_from(pt, a.op, qj.x, qj.y, s, e); out[2 * n] = s - gap; out[2 * n + 1] = e - gap; }
        n++;
      }
    }
  }
  return n;
}

struct OffsetFn {
  OffsetArgs a; long long *out, *firstInverted;
  __device__ __forceinline__ void operator()(long long t, long long p, int r) const
  {
    long long s, e;
    if (!a.fromQuery) offset_from(ref_point(a, r), a.op, a.q.tri[3 * t + 1], a.q.tri[3 * t + 2], s, e);
    else { const int4 v = a.refEnds[r]; offset_from(query_point(a, t), a.op, v.x, v.w, s, e); }
    out[2 * p] = s; out[2 * p + 1] = e;
    if (s > e) atomicMin(firstInverted, p);
  }
};

struct GapsCountFn {
  OffsetArgs a; long long *cnt;
  __device__ __forceinline__ void operator()(long long t, long long p, int r) const { cnt[p] = gaps_walk(a, t, r, nullptr); }
};

struct GapsEmitFn {
  OffsetArgs a; const long long *eoff; long long *out;
  __device__ __forceinline__ void operator()(long long t, long long p, int r) const { gaps_walk(a, t, r, out + 2 * eoff[p]); }
};

// one lane per query over its segment; longer segments go to the list big (count, then query indices relative to q0)
template <class F>
__global__ __launch_bounds__(256) void seg_small_kernel(long long q0, long long q1, const long long *__restrict__ off, const int *__restrict__ pairs,
                                                        long long nPairs, unsigned *__restrict__ big, F f)
{
  const long long t = q0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= q1) return;
  const long long o0 = off[q0], b = off[t] - o0, e = min(off[t + 1] - o0, nPairs);
  if (e - b > kOffSmallSeg) { const unsigned at = atomicAdd(big, 1u); big[1 + at] = (unsigned)(t - q0); return; }
  for (long long p = b; p < e; p++) f(t, p, pairs[p]);
}

// one block per listed query, its lanes striding over the segment
template <class F>
__global__ __launch_bounds__(256) void seg_big_kernel(long long q0, const long long *__restrict__ off, const int *__restrict__ pairs, long long nPairs,
                                                      const unsigned *__restrict__ big, F f)
{
  const unsigned nBig = big[0];
  const long long o0 = off[q0];
  for (unsigned k = blockIdx.x; k < nBig; k += gridDim.x) {
    const long long t = q0 + big[1 + k];
    const long long b = off[t] - o0, e = min(off[t + 1] - o0, nPairs);
    for (long long p = b + threadIdx.x; p < e; p += blockDim.x) f(t, p, pairs[p]);
  }
}

__global__ __launch_bounds__(256) void ref_ends_kernel(const int2 *__restrict__ env, RegionBlocks rb, long long m, int4 *__restrict__ out)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int2 b = rb.blkOf ? rb.blkOf[r] : make_int2(0, 0);
  if (b.y) { const int2 f = rb.iv[b.x], l = rb.iv[b.x + b.y - 1]; out[r] = make_int4(f.x, f.y, l.x, l.y); }
  else { const int2 v = env[r]; out[r] = make_int4(v.x, v.y, v.x, v.y); }
}

inline unsigned grid_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

template <class F>
hipError_t launch_segments(long long q0, long long q1, const long long *off, const int *pairs, long long nPairs, unsigned *big, const F &f, hipStream_t st)
{
  if (q1 <= q0 || nPairs <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(big, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(seg_small_kernel<F>, dim3(grid_of(q1 - q0, 256)), dim3(256), 0, st, q0, q1, off, pairs, nPairs, big, f);
  hipLaunchKernelGGL(seg_big_kernel<F>, dim3(1024), dim3(256), 0, st, q0, off, pairs, nPairs, (const unsigned *)big, f);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_pair_offsets(const OffsetArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                               long long *out, long long *firstInverted, unsigned *big, hipStream_t st)
{
  return launch_segments(q0, q1, off, pairs, nPairs, big, OffsetFn{a, out, firstInverted}, st);
}

hipError_t launch_pair_gaps_count(const OffsetArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                                  long long *cnt, unsigned *big, hipStream_t st)
{
  return launch_segments(q0, q1, off, pairs, nPairs, big, GapsCountFn{a, cnt}, st);
}

hipError_t launch_pair_gaps_emit(const OffsetArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                                 const long long *eoff, long long *out, unsigned *big, hipStream_t st)
{
  return launch_segments(q0, q1, off, pairs, nPairs, big, GapsEmitFn{a, eoff, out}, st);
}

hipError_t launch_ref_ends(const int2 *env, const RegionBlocks &rb, long long m, int4 *refEnds, hipStream_t st)
{
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(ref_ends_kernel, dim3(grid_of(m, 256)), dim3(256), 0, st, env, rb, m, refEnds);
  return hipGetLastError();
}

}  // namespace gtx
