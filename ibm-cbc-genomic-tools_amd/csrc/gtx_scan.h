// gtx_scan.h -- the prefix step of every "count per tile, prefix, emit" pass, defined once: over a wave (wave_inclusive, and its DPP
// form for sums), over a block with one value per thread (tile_exclusive), and over an array by one block (run_exclusive_sum).
// Device code.  The barriers and the LDS named in a function's comment are part of its contract: the kernels around these are written
// against them.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace gtxscan {

// The scans over an array run in one block, each thread over a run of consecutive entries: the loads of a run go out kPartBatch at a
// time (they do not depend on one another; one at a time the kernel is a chain of memory latencies).
constexpr int kPartBatch = 8;

struct plus { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };

// v of the lane o places below in the wave (undefined for the lowest o lanes); T of whole 32-bit words, a vector of them included
template <class T>
__device__ __forceinline__ T lane_up(T v, int o)
{
  static_assert(sizeof(T) % sizeof(int) == 0, "whole words");
  int w[sizeof(T) / sizeof(int)];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (unsigned k = 0; k < sizeof(T) / sizeof(int); k++) w[k] = __shfl_up(w[k], o);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}

// op over v of lanes 0 .. this one of the wave, in lane order: op(lower lanes, mine), so op need only be associative.  The shuffle
// ladder: registers only, no barrier, no LDS.  Every lane of the wave calls it (a lane that stays away leaves what it would have
// passed up undefined).  T as for lane_up.
template <class T, class OP = plus>
__device__ __forceinline__ T wave_inclusive(T v, OP op = OP())
{
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const T up = lane_up(v, o); if (lane >= o) v = op(up, v); }
  return v;
}

// The sum of v over lanes 0 .. this one, DPP only (no LDS): Hillis-Steele inside each row of 16 lanes (row_shr 1, 2, 4, 8 with zero
// fill), then row_bcast15 hands a row's total to the next odd row and row_bcast31 the total of lanes 0..31 to the upper half.  Call
// with all lanes active: a lane that is masked off reads as 0 to the rows behind it.
__device__ __forceinline__ int wave_inclusive_dpp(int v)
{
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}
__device__ __forceinline__ unsigned wave_inclusive_dpp(unsigned v) { return (unsigned)wave_inclusive_dpp((int)v); }

// the same for 64-bit values: both halves travel by DPP, the add carries
__device__ __forceinline__ unsigned long long wave_inclusive_dpp(unsigned long long v)
{
  typedef unsigned long long u64;
#define GTX_DPP64(ctrl, rmask, bc)                                                                                  \
  v += ((u64)(unsigned)__builtin_amdgcn_update_dpp(0, (int)(v >> 32), ctrl, rmask, 0xf, bc) << 32) |                \
       (u64)(unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, ctrl, rmask, 0xf, bc)
  GTX_DPP64(0x111, 0xf, true); GTX_DPP64(0x112, 0xf, true); GTX_DPP64(0x114, 0xf, true); GTX_DPP64(0x118, 0xf, true);
  GTX_DPP64(0x142, 0xa, false); GTX_DPP64(0x143, 0xc, false);
#undef GTX_DPP64
  return v;
}

// op over v of the threads in front of this one in a block of THREADS threads (64, or a multiple of it), in thread order; `identity`
// for thread 0.  Every thread calls it.  T: an integer, a vector of them for several sums at once, or with an op of its own any struct
// of whole 32-bit words.  One wave: registers only, no barrier, and waveSum is not touched.  More waves: waveSum[THREADS / 64] in LDS
// and exactly one barrier, which the caller may rely on for what it wrote to LDS in front of it.  With `total`, *total = op over the
// whole block, in every thread (behind that barrier; no further one).  waveSum is read behind the barrier: the caller has a barrier
// between this and its next write to waveSum, a second call with the same array included.
template <int THREADS, class T, class OP = plus>
__device__ __forceinline__ T tile_exclusive(T v, T *waveSum, T *total = nullptr, T identity = T{}, OP op = OP())
{
  static_assert(THREADS >= 64 && THREADS % 64 == 0, "whole waves");
  const int lane = threadIdx.x & 63;
  const T incl = wave_inclusive(v, op);
  constexpr bool kSum = std::is_same<OP, plus>::value;                // + has an inverse and commutes: the short form of both steps
  T at;
  if constexpr (kSum) at = incl - v;
  else { at = lane_up(incl, 1); if (lane == 0) at = identity; }
  if constexpr (THREADS > 64) {
    const int w = threadIdx.x >> 6;
    if (lane == 63) waveSum[w] = incl;
    __syncthreads();
    if constexpr (kSum) for (int k = 0; k < w; k++) at += waveSum[k];
    else for (int k = w - 1; k >= 0; k--) at = op(waveSum[k], at);    // the waves in front, nearest first: each goes in front of what is there
    if (total) {
      T all = waveSum[0];
#pragma unroll 4                                                     // (16 wide values read at once cost a 1024-thread kernel its occupancy)
      for (int k = 1; k < THREADS / 64; k++) all = op(all, waveSum[k]);
      *total = all;
    }
  } else if (total) {
    int word[sizeof(T) / sizeof(int)];
    __builtin_memcpy(word, &incl, sizeof(T));
#pragma unroll
    for (unsigned k = 0; k < sizeof(T) / sizeof(int); k++) word[k] = __shfl(word[k], 63);
    __builtin_memcpy(total, word, sizeof(T));
  }
  return at;
}

// out[k] = in[0] + .. + in[k - 1] for k < n, by one block of THREADS threads, each over a run of consecutive entries; the sum of all n
// is returned in every thread, and out[n] is the caller's to write.  out may be in itself; they may lie in LDS.  IN: 32 or 64 bits;
// OUT: IN, or long long; the sums are taken in OUT, so an in-place 32-bit scan wraps modulo 2^32.  waveSum[THREADS / 64] in LDS (not
// touched by one wave).  Every thread calls it.  Barriers: tile_exclusive's one between the two turns, and one at the end: behind it
// every thread may read out[0 .. n) and waveSum is free.  The caller has a barrier (or a kernel boundary) between the writes of in and
// this.
template <int THREADS, class IN, class OUT>
__device__ __forceinline__ OUT run_exclusive_sum(const IN *in, long long n, OUT *out, OUT *waveSum)
{
  typedef long long i64;
  static_assert((sizeof(IN) == 4 || sizeof(IN) == 8) && (sizeof(OUT) == sizeof(IN) || sizeof(OUT) == 8), "32 or 64 bits, never narrowed");
  const i64 per = (n + THREADS - 1) / THREADS, b = min((i64)threadIdx.x * per, n), e = min(b + per, n);
  OUT a = 0;
  for (i64 k = b; k < e; k += kPartBatch) {
    IN v[kPartBatch];
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) v[j] = k + j < e ? in[k + j] : (IN)0;
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) a += (OUT)v[j];
  }
  OUT all;
  OUT run = tile_exclusive<THREADS>(a, waveSum, &all);
  for (i64 k = b; k < e; k += kPartBatch) {
    IN v[kPartBatch];
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) v[j] = k + j < e ? in[k + j] : (IN)0;
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) if (k + j < e) { out[k + j] = run; run += (OUT)v[j]; }
  }
  __syncthreads();
  return all;
}

}  // namespace gtxscan
