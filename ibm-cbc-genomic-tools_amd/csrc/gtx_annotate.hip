// Kernels of the annotate pass (see gtx_annotate.h).
#include "gtx_annotate.h"

namespace gtx {
namespace {

constexpr int kAnnThreads = 256, kAnnWave = 64, kAnnWaves = kAnnThreads / kAnnWave;

// PrintAnnotations (gtools/genomic_overlaps.cpp:271-275) of the query [s, e] against ordinal r: is the pair printed, and its value
__device__ __forceinline__ bool pair_value(const AnnotateArgs &a, long long s, long long e, int r, long long &v)
{
  if (r < 0 || r >= a.nRefs) return false;
  const int4 x = a.refEnds[r];
  const Point pt{make_int2(x.x, x.y), make_int2(x.z, x.w), a.refStrand != nullptr && a.refStrand[r] == '-'};
  long long so, eo;
  offset_from(pt, r < a.nPrimary ? a.opPrimary : a.opRest, s, e, so, eo);
  if (a.mode == ANN_CENTER) { v = so + eo; return v >= 0; }          // (double)(so + eo) / 2 < 0 is skipped: -0.5 too
  v = so;
  return true;
}

// one lane per query; a longer segment goes to the list big (count, then query indices relative to q0)
__global__ __launch_bounds__(kAnnThreads) void annotate_count_small_kernel(AnnotateArgs a, long long q0, long long q1, const long long *__restrict__ off,
                                                                           const int *__restrict__ pairs, long long nPairs, long long *__restrict__ cnt,
                                                                           unsigned *__restrict__ big)
{
  const long long t = q0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= q1) return;
  const long long o0 = off[q0], b = min(off[t] - o0, nPairs), e = min(off[t + 1] - o0, nPairs);
  if (e - b > kOffSmallSeg) { const unsigned at = atomicAdd(big, 1u); big[1 + at] = (unsigned)(t - q0); return; }
  const long long s = a.tri[3 * t + 1], x = a.tri[3 * t + 2];
  long long c = 0, v;
  for (long long p = b; p < e; p++) c += pair_value(a, s, x, pairs[p], v) ? 1 : 0;
  cnt[t - q0] = c;
}

// one block per listed query
__global__ __launch_bounds__(kAnnThreads) void annotate_count_big_kernel(AnnotateArgs a, long long q0, const long long *__restrict__ off,
                                                                         const int *__restrict__ pairs, long long nPairs, long long *__restrict__ cnt,
                                                                         const unsigned *__restrict__ big)
{
  __shared__ long long wsum[kAnnWaves];
  const unsigned nBig = big[0];
  const long long o0 = off[q0];
  const int lane = threadIdx.x % kAnnWave, w = threadIdx.x / kAnnWave;
  for (unsigned k = blockIdx.x; k < nBig; k += gridDim.x) {
    const long long t = q0 + big[1 + k];
    const long long b = min(off[t] - o0, nPairs), e = min(off[t + 1] - o0, nPairs);
    const long long s = a.tri[3 * t + 1], x = a.tri[3 * t + 2];
    long long c = 0, v;                                                   // the same in every lane of a wave
    for (long long p0 = b; p0 < e; p0 += kAnnThreads) {
      const long long p = p0 + threadIdx.x;
      const bool keep = p < e && pair_value(a, s, x, pairs[p], v);
      c += __popcll(__ballot(keep));
    }
    if (lane == 0) wsum[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) { long long z = 0; for (int i = 0; i < kAnnWaves; i++) z += wsum[i]; cnt[t - q0] = z; }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kAnnThreads) void annotate_emit_small_kernel(AnnotateArgs a, long long q0, long long q1, const long long *__restrict__ off,
                                                                          const int *__restrict__ pairs, long long nPairs, const long long *__restrict__ koff,
                                                                          int *__restrict__ keptRef, long long *__restrict__ keptValue, long long cap)
{
  const long long t = q0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= q1) return;
  const long long o0 = off[q0], b = min(off[t] - o0, nPairs), e = min(off[t + 1] - o0, nPairs);
  if (e - b > kOffSmallSeg) return;                                       // (listed by the count pass)
  const long long s = a.tri[3 * t + 1], x = a.tri[3 * t + 2];
  long long o = koff[t - q0], v;
  for (long long p = b; p < e && o < cap; p++) {
    const int r = pairs[p];
    if (pair_value(a, s, x, r, v)) { keptRef[o] = r; keptValue[o] = v; o++; }
  }
}

// one block per listed query: tiles of 256 pairs, each kept pair behind those of its tile before it (ballot ranks inside a wave, the
// waves' totals through LDS) and the tiles before
__global__ __launch_bounds__(kAnnThreads) void annotate_emit_big_kernel(AnnotateArgs a, long long q0, const long long *__restrict__ off,
                                                                        const int *__restrict__ pairs, long long nPairs, const long long *__restrict__ koff,
                                                                        int *__restrict__ keptRef, long long *__restrict__ keptValue, long long cap,
                                                                        const unsigned *__restrict__ big)
{
  __shared__ int wsum[kAnnWaves];
  const unsigned nBig = big[0];
  const long long o0 = off[q0];
  const int lane = threadIdx.x % kAnnWave, w = threadIdx.x / kAnnWave;
  for (unsigned k = blockIdx.x; k < nBig; k += gridDim.x) {
    const long long t = q0 + big[1 + k];
    const long long b = min(off[t] - o0, nPairs), e = min(off[t + 1] - o0, nPairs);
    const long long s = a.tri[3 * t + 1], x = a.tri[3 * t + 2];
    long long base = koff[t - q0];
    for (long long p0 = b; p0 < e && base < cap; p0 += kAnnThreads) {    // (base is the same in every lane)
      const long long p = p0 + threadIdx.x;
      long long v = 0;
      const int r = p < e ? pairs[p] : -1;
      const bool keep = p < e && pair_value(a, s, x, r, v);
      const unsigned long long m = __ballot(keep);
      if (lane == 0) wsum[w] = __popcll(m);
      __syncthreads();
      int before = __popcll(m & ((1ull << lane) - 1)), total = 0;
      for (int i = 0; i < kAnnWaves; i++) { if (i < w) before += wsum[i]; total += wsum[i]; }
      const long long o = base + before;
      if (keep && o < cap) { keptRef[o] = r; keptValue[o] = v; }
      base += total;
      __syncthreads();
    }
  }
}

inline unsigned grid_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_annotate_count(const AnnotateArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                                 long long *cnt, unsigned *big, hipStream_t st)
{
  if (q1 <= q0) return hipSuccess;
  hipError_t e = hipMemsetAsync(big, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(annotate_count_small_kernel, dim3(grid_of(q1 - q0, kAnnThreads)), dim3(kAnnThreads), 0, st, a, q0, q1, off, pairs, nPairs, cnt, big);
  hipLaunchKernelGGL(annotate_count_big_kernel, dim3(1024), dim3(kAnnThreads), 0, st, a, q0, off, pairs, nPairs, cnt, (const unsigned *)big);
  return hipGetLastError();
}

hipError_t launch_annotate_emit(const AnnotateArgs &a, long long q0, long long q1, const long long *off, const int *pairs, long long nPairs,
                                const long long *koff, int *keptRef, long long *keptValue, long long cap, const unsigned *big, hipStream_t st)
{
  if (q1 <= q0 || cap <= 0) return hipSuccess;
  hipLaunchKernelGGL(annotate_emit_small_kernel, dim3(grid_of(q1 - q0, kAnnThreads)), dim3(kAnnThreads), 0, st, a, q0, q1, off, pairs, nPairs, koff, keptRef,
                     keptValue, cap);
  hipLaunchKernelGGL(annotate_emit_big_kernel, dim3(1024), dim3(kAnnThreads), 0, st, a, q0, off, pairs, nPairs, koff, keptRef, keptValue, cap, big);
  return hipGetLastError();
}

}  // namespace gtx
