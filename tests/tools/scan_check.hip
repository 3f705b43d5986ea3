// scan_check -- the scan primitives of csrc/gtx_scan.h against plain host loops, at their seams: run_exclusive_sum at every n around a
// wave, a block and a load batch, from 32 to 64 bits and in place, in global memory and in LDS; tile_exclusive with its total, with + and with a segmented max
// (an op that does not commute); wave_inclusive against wave_inclusive_dpp.  Prints the first case that differs and exits non-zero.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include <vector>
#include "gtx_scan.h"

typedef unsigned long long u64;
typedef long long i64;

#define CHECK(call)                                                                                            \
  do {                                                                                                         \
    const hipError_t e_ = (call);                                                                              \
    if (e_ != hipSuccess) { fprintf(stderr, "scan_check: %s: %s\n", #call, hipGetErrorString(e_)); exit(2); } \
  } while (0)

static u64 rngState = 0x9e3779b97f4a7c15ull;
static u64 rng() { rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17; return rngState; }

// ---- run_exclusive_sum ----
// out [n], all [THREADS]: what every thread got back
template <int THREADS, class IN, class OUT>
__global__ __launch_bounds__(THREADS) void run_kernel(const IN *in, i64 n, OUT *out, OUT *all)
{
  __shared__ OUT waveSum[THREADS / 64];
  all[threadIdx.x] = gtxscan::run_exclusive_sum<THREADS>(in, n, out, waveSum);
}

// the same in place over an array in LDS (the tail of scan_own_kernel): in [n] goes in, its sums come back in out [n]; n <= kLdsN
constexpr int kLdsN = 4096;
template <int THREADS, class T>
__global__ __launch_bounds__(THREADS) void run_lds_kernel(const T *in, int n, T *out, T *all)
{
  __shared__ T v[kLdsN];
  __shared__ T waveSum[THREADS / 64];
  for (int k = threadIdx.x; k < n; k += THREADS) v[k] = in[k];
  __syncthreads();
  all[threadIdx.x] = gtxscan::run_exclusive_sum<THREADS>(v, n, v, waveSum);
  for (int k = threadIdx.x; k < n; k += THREADS) out[k] = v[k];      // (behind the primitive's last barrier)
}

static const i64 kMaxN = 24 * 1024 + 5;
static void *dIn, *dOut, *dAll;                                       // 8 (kMaxN + 1), 8 (kMaxN + 1) and 8 x 1024 bytes

// kind 0: values within 16 of 2^32 - 1 (a 32-bit sum of two is wrong); 1: 40 random bits; 2: all bits random (the sums wrap)
// LDS (with INPLACE): the array is staged in LDS and scanned there (run_lds_kernel)
template <int THREADS, class IN, class OUT, bool INPLACE, bool LDS = false>
static bool run_case(const char *name, i64 n, int kind)
{
  static_assert(!LDS || (INPLACE && std::is_same<IN, OUT>::value), "the LDS case is in place");
  std::vector<IN> in(n + 1);
  std::vector<OUT> want(n + 1), got(n + 1), all(THREADS);
  OUT sum = 0;
  for (i64 k = 0; k < n; k++) {
    in[k] = kind == 0 ? (IN)(0xffffffffull - (rng() & 15)) : kind == 1 ? (IN)(rng() >> 24) : (IN)rng();
    want[k] = sum; sum += (OUT)in[k];
  }
  const OUT guard = (OUT)0x5a5a5a5a5a5a5a5aull;                       // behind the last entry: not the primitive's to write
  in[n] = (IN)guard; want[n] = guard;
  IN *src = INPLACE && !LDS ? (IN *)dOut : (IN *)dIn;
  if (!INPLACE || LDS) { std::vector<OUT> fill(n + 1, guard); CHECK(hipMemcpy(dOut, fill.data(), sizeof(OUT) * (n + 1), hipMemcpyHostToDevice)); }
  CHECK(hipMemcpy(src, in.data(), sizeof(IN) * (n + 1), hipMemcpyHostToDevice));
  if constexpr (LDS) hipLaunchKernelGGL((run_lds_kernel<THREADS, OUT>), dim3(1), dim3(THREADS), 0, 0, (const OUT *)src, (int)n, (OUT *)dOut, (OUT *)dAll);
  else hipLaunchKernelGGL((run_kernel<THREADS, IN, OUT>), dim3(1), dim3(THREADS), 0, 0, (const IN *)src, n, (OUT *)dOut, (OUT *)dAll);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(got.data(), dOut, sizeof(OUT) * (n + 1), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(all.data(), dAll, sizeof(OUT) * THREADS, hipMemcpyDeviceToHost));
  for (i64 k = 0; k <= n; k++)
    if (got[k] != want[k]) {
      printf("run_exclusive_sum<%d> %s n=%lld: out[%lld] = %lld, expected %lld%s\n", THREADS, name, n, k, (i64)got[k], (i64)want[k], k == n ? " (the entry behind the last was written)" : "");
      return false;
    }
  for (int t = 0; t < THREADS; t++)
    if (all[t] != sum) { printf("run_exclusive_sum<%d> %s n=%lld: thread %d got the total %lld, expected %lld\n", THREADS, name, n, t, (i64)all[t], (i64)sum); return false; }
  return true;
}

template <int THREADS>
static bool run_cases()
{
  const i64 ns[] = {0, 1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 8 * THREADS - 1, 8 * THREADS, 8 * THREADS + 1, 24 * THREADS + 5};
  for (const i64 n : ns) {
    if (!run_case<THREADS, unsigned, i64, false>("unsigned -> int64", n, 0)) return false;
    if (!run_case<THREADS, u64, i64, false>("uint64 -> int64", n, 1)) return false;
    if (!run_case<THREADS, unsigned, unsigned, true>("unsigned in place", n, 2)) return false;
    if (!run_case<THREADS, u64, u64, true>("uint64 in place", n, 2)) return false;
    if (n > kLdsN) continue;
    if (!run_case<THREADS, unsigned, unsigned, true, true>("unsigned in place in LDS", n, 2)) return false;
    if (!run_case<THREADS, u64, u64, true, true>("uint64 in place in LDS", n, 2)) return false;
  }
  return true;
}

// ---- tile_exclusive ----
struct Seg { int f, m; };                                             // {a segment begins here or in front, the largest value since}
struct SegOp { __host__ __device__ Seg operator()(Seg a, Seg b) const { return Seg{a.f | b.f, b.f ? b.m : (a.m > b.m ? a.m : b.m)}; } };
static const Seg kSegIdentity = {0, INT_MIN};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void tile_kernel(const unsigned *v, unsigned *at, unsigned *total, const Seg *sv, Seg *sat, Seg *stotal)
{
  __shared__ unsigned waveSum[THREADS / 64];
  __shared__ Seg waveSeg[THREADS / 64];
  unsigned tot;
  at[threadIdx.x] = gtxscan::tile_exclusive<THREADS>(v[threadIdx.x], waveSum, &tot);
  total[threadIdx.x] = tot;
  Seg stot;
  sat[threadIdx.x] = gtxscan::tile_exclusive<THREADS>(sv[threadIdx.x], waveSeg, &stot, Seg{0, INT_MIN}, SegOp());
  stotal[threadIdx.x] = stot;
}

template <int THREADS>
static bool tile_case(int round)
{
  std::vector<unsigned> v(THREADS), at(THREADS), total(THREADS);
  std::vector<Seg> sv(THREADS), sat(THREADS), stotal(THREADS);
  for (int t = 0; t < THREADS; t++) {
    v[t] = (unsigned)rng();
    // flags about one in 2^round lanes, so that segments reach over lanes, over waves and, in the last rounds, over the whole block
    sv[t].f = (rng() & ((1u << round) - 1)) == 0; sv[t].m = (int)(unsigned)rng();
  }
  unsigned *dV = (unsigned *)dIn, *dAt = dV + 1024, *dTot = dV + 2048;
  Seg *dSv = (Seg *)dOut, *dSat = dSv + 1024, *dStot = dSv + 2048;
  CHECK(hipMemcpy(dV, v.data(), sizeof(unsigned) * THREADS, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dSv, sv.data(), sizeof(Seg) * THREADS, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(tile_kernel<THREADS>, dim3(1), dim3(THREADS), 0, 0, (const unsigned *)dV, dAt, dTot, (const Seg *)dSv, dSat, dStot);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(at.data(), dAt, sizeof(unsigned) * THREADS, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(total.data(), dTot, sizeof(unsigned) * THREADS, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(sat.data(), dSat, sizeof(Seg) * THREADS, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(stotal.data(), dStot, sizeof(Seg) * THREADS, hipMemcpyDeviceToHost));
  unsigned sum = 0; Seg fold = kSegIdentity;
  for (int t = 0; t < THREADS; t++) {
    if (at[t] != sum) { printf("tile_exclusive<%d> +, round %d: thread %d got %u, expected %u\n", THREADS, round, t, at[t], sum); return false; }
    if (sat[t].f != fold.f || sat[t].m != fold.m) {
      printf("tile_exclusive<%d> segmented max, round %d: thread %d got {%d, %d}, expected {%d, %d}\n", THREADS, round, t, sat[t].f, sat[t].m, fold.f, fold.m);
      return false;
    }
    sum += v[t]; fold = SegOp()(fold, sv[t]);
  }
  for (int t = 0; t < THREADS; t++) {
    if (total[t] != sum) { printf("tile_exclusive<%d> +, round %d: thread %d got the total %u, expected %u\n", THREADS, round, t, total[t], sum); return false; }
    if (stotal[t].f != fold.f || stotal[t].m != fold.m) {
      printf("tile_exclusive<%d> segmented max, round %d: thread %d got the total {%d, %d}, expected {%d, %d}\n", THREADS, round, t, stotal[t].f, stotal[t].m, fold.f, fold.m);
      return false;
    }
  }
  return true;
}

template <int THREADS>
static bool tile_cases()
{
  for (int round = 0; round <= 12; round++) if (!tile_case<THREADS>(round)) return false;
  return true;
}

// ---- wave_inclusive against wave_inclusive_dpp ----
constexpr int kWaveThreads = 256;
__global__ __launch_bounds__(kWaveThreads) void wave_kernel(const int *v32, const u64 *v64, int *shfl32, int *dpp32, u64 *shfl64, u64 *dpp64)
{
  const int t = threadIdx.x;
  shfl32[t] = gtxscan::wave_inclusive(v32[t]); dpp32[t] = gtxscan::wave_inclusive_dpp(v32[t]);
  shfl64[t] = gtxscan::wave_inclusive(v64[t]); dpp64[t] = gtxscan::wave_inclusive_dpp(v64[t]);
}

static bool wave_case()
{
  std::vector<int> v32(kWaveThreads), s32(kWaveThreads), d32(kWaveThreads);
  std::vector<u64> v64(kWaveThreads), s64(kWaveThreads), d64(kWaveThreads);
  for (int t = 0; t < kWaveThreads; t++) { v32[t] = (int)(unsigned)rng(); v64[t] = rng(); }   // signed values of both signs; the sums wrap
  int *dV32 = (int *)dIn, *dS32 = dV32 + 1024, *dD32 = dV32 + 2048;
  u64 *dV64 = (u64 *)dOut, *dS64 = dV64 + 1024, *dD64 = dV64 + 2048;
  CHECK(hipMemcpy(dV32, v32.data(), sizeof(int) * kWaveThreads, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dV64, v64.data(), sizeof(u64) * kWaveThreads, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(wave_kernel, dim3(1), dim3(kWaveThreads), 0, 0, (const int *)dV32, (const u64 *)dV64, dS32, dD32, dS64, dD64);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(s32.data(), dS32, sizeof(int) * kWaveThreads, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(d32.data(), dD32, sizeof(int) * kWaveThreads, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(s64.data(), dS64, sizeof(u64) * kWaveThreads, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(d64.data(), dD64, sizeof(u64) * kWaveThreads, hipMemcpyDeviceToHost));
  unsigned sum32 = 0; u64 sum64 = 0;
  for (int t = 0; t < kWaveThreads; t++) {
    if (t % 64 == 0) { sum32 = 0; sum64 = 0; }
    sum32 += (unsigned)v32[t]; sum64 += v64[t];
    if (s32[t] != (int)sum32 || d32[t] != (int)sum32) { printf("wave scan, 32 bits, thread %d: shuffle %d, DPP %d, expected %d\n", t, s32[t], d32[t], (int)sum32); return false; }
    if (s64[t] != sum64 || d64[t] != sum64) { printf("wave scan, 64 bits, thread %d: shuffle %lld, DPP %lld, expected %lld\n", t, (i64)s64[t], (i64)d64[t], (i64)sum64); return false; }
  }
  return true;
}

int main()
{
  CHECK(hipMalloc(&dIn, 8 * (kMaxN + 1)));
  CHECK(hipMalloc(&dOut, 8 * (kMaxN + 1)));
  CHECK(hipMalloc(&dAll, 8 * 1024));
  const bool ok = run_cases<64>() && run_cases<256>() && run_cases<1024>() && tile_cases<64>() && tile_cases<256>() && tile_cases<1024>() && wave_case();
  CHECK(hipFree(dIn)); CHECK(hipFree(dOut)); CHECK(hipFree(dAll));
  if (ok) printf("scan_check ok\n");
  return ok ? 0 : 1;
}
