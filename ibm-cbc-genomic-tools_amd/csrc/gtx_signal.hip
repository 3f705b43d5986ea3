// Kernel of the signal bins (see gtx_signal.h).  Built with -ffp-contract=off.
#include <algorithm>
#include <climits>
#include "gtx_signal.h"
#include "gtx_join_walk.h"
#include "gtx_offset.h"

namespace gtx {
namespace {

constexpr int kSignalThreads = 256;
enum { S_PAIRS, S_BINNED, S_DROPPED, S_ABS, S_NOCLASS, S_DEGEN, S_N };

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
  for (int d = warpSize / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;
}

// kLds: the profile's row in LDS (nBins <= kSignalLdsBins), flushed at the end; otherwise every pair adds in HBM
template <bool kLds>
__global__ __launch_bounds__(kSignalThreads) void signal_bins_kernel(SignalArgs a, unsigned long long *__restrict__ bins, SignalInfo *info)
{
  extern __shared__ unsigned long long hist[];
  __shared__ unsigned long long red[S_N];
  const int tid = threadIdx.x;
  if (tid < S_N) red[tid] = 0;
  if (kLds) for (long long i = tid; i < a.nBins; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  unsigned long long cnt[S_N] = {0, 0, 0, 0, 0, 0};
  long long firstInv = LLONG_MAX;
  const double span = a.binMax - a.binMin, nb = (double)a.nBins;
  for (long long t = (long long)blockIdx.x * blockDim.x + tid; t < a.q.n; t += (long long)gridDim.x * blockDim.x) {
    bool noClass, degenerate;
    const Query qq = load_query(a.q, t, a.ix, a.mode, noClass, degenerate);
    cnt[S_NOCLASS] += noClass; cnt[S_DEGEN] += degenerate;
    if (!qq.match) continue;
    const long long w = a.w ? a.w[t] : 1;
    const int2 f = a.q.blk ? a.q.iv[qq.blk.x] : make_int2(qq.s, qq.e);       // qreg->I.front()
    walk(qq, a.q.iv, a.ix, a.rb, a.mode, [&](int r) {
      cnt[S_PAIRS]++;
      const int4 v = a.refEnds[r];
      const Point pt{make_int2(v.x, v.y), make_int2(v.z, v.w), a.refStrand != nullptr && a.refStrand[r] == '-'};
      long long s, e;
      offset_from(pt, OFF_5P, f.x, f.y, s, e);
      if (s > e) { firstInv = min(firstInv, t); return; }                   // the reference's exit; the caller reports it
      const double len = a.refLen ? (double)(unsigned long long)a.refLen[r] : 1.0;
      const double x = (double)(s + e) / 2 / len + a.binMin;
      const double z = (x - a.binMin) / span;
      if (!(z >= 0 && z < 1)) return;
      const int bin = (int)(nb * z);
      if (bin >= a.nBins) { cnt[S_DROPPED]++; return; }
      cnt[S_BINNED]++; cnt[S_ABS] += (unsigned long long)(w < 0 ? -w : w);
      if (kLds) atomicAdd(&hist[bin], (unsigned long long)w);
      else atomicAdd(&bins[(a.perRef ? (long long)r * a.nBins : 0) + bin], (unsigned long long)w);
    });
  }
  for (int k = 0; k < S_N; k++) {
    const unsigned long long s = wave_sum(cnt[k]);
    if ((tid & (warpSize - 1)) == 0 && s) atomicAdd(&red[k], s);
  }
  if (firstInv != LLONG_MAX) atomicMin(&info->firstInverted, firstInv);
  __syncthreads();
  if (kLds) for (long long i = tid; i < a.nBins; i += blockDim.x) if (hist[i]) atomicAdd(&bins[i], hist[i]);
  if (tid == 0) {
    unsigned long long *dst[S_N] = {&info->pairs, &info->binned, &info->dropped, &info->absWeight, &info->noClass, &info->degenerate};
    for (int k = 0; k < S_N; k++) if (red[k]) atomicAdd(dst[k], red[k]);
  }
}

}  // namespace

hipError_t launch_signal_bins(const SignalArgs &a, unsigned long long *bins, SignalInfo *info, int nCU, hipStream_t st)
{
  if (a.q.n <= 0) return hipSuccess;
  const bool lds = !a.perRef && a.nBins <= kSignalLdsBins;
  const size_t smem = lds ? sizeof(unsigned long long) * (size_t)std::max<long long>(a.nBins, 1) : 0;
  // one wave of resident blocks: the lanes stride over the reads, so a block beyond what the CUs hold would run as a tail
  int perCU = 0;
  hipError_t e = lds ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, signal_bins_kernel<true>, kSignalThreads, smem)
                     : hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, signal_bins_kernel<false>, kSignalThreads, 0);
  if (e != hipSuccess) return e;
  const long long need = (a.q.n + kSignalThreads - 1) / kSignalThreads;
  const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(need, (long long)std::max(perCU, 1) * std::max(nCU, 1)));
  if (lds) hipLaunchKernelGGL(signal_bins_kernel<true>, dim3(grid), dim3(kSignalThreads), smem, st, a, bins, info);
  else hipLaunchKernelGGL(signal_bins_kernel<false>, dim3(grid), dim3(kSignalThreads), 0, st, a, bins, info);
  return hipGetLastError();
}

}  // namespace gtx
