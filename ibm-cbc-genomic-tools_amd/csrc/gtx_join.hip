// Kernels of the overlap join (see gtx_join.h).  One lane per query for the two walks: a query's candidates are a contiguous
// run of the envelope index that the lane reads from the top down, so lanes of sorted queries read neighbouring runs.
#include <climits>
#include "gtx_join.h"
#include "gtx_join_walk.h"
#include "gtx_scan.h"

namespace gtx {
namespace {

__global__ __launch_bounds__(256) void join_count_kernel(JoinQueries q, PairIndex ix, RegionBlocks rb, int mode, long long *__restrict__ off, JoinInfo *info)
{
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= q.n) return;
  bool noClass, degenerate;
  const Query qq = load_query(q, t, ix, mode, noClass, degenerate);
  long long c = 0;
  if (qq.match) walk(qq, q.iv, ix, rb, mode, [&](int) { c++; });
  off[t] = c;
  if (noClass) atomicAdd((unsigned long long *)&info->noClass, 1ull);
  if (degenerate) { atomicAdd((unsigned long long *)&info->degenerate, 1ull); atomicMin(&info->firstDegenerate, t); }
  if ((mode & JOIN_CHECK) && t > 0) {
    const int pc = q.tri[3 * t - 3], ps = q.tri[3 * t - 2];
    if (qq.cls < pc || (qq.cls == pc && qq.s < ps)) atomicMin(&info->firstUnsorted, t);
  }
}

__global__ __launch_bounds__(256) void join_emit_kernel(JoinQueries q, long long q0, long long q1, PairIndex ix, RegionBlocks rb, int mode,
                                                        const long long *__restrict__ off, int *__restrict__ pairs, JoinInfo *info)
{
  const long long t = q0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= q1) return;
  const long long o = off[t] - off[q0], c = off[t + 1] - off[t];
  if (c == 0) return;
  bool noClass, degenerate;
  const Query qq = load_query(q, t, ix, mode, noClass, degenerate);
  long long j = 0;
  int *seg = pairs + o;
  if (qq.match) walk(qq, q.iv, ix, rb, mode, [&](int r) { if (j < c) seg[c - 1 - j] = r; j++; });
  if (j != c) atomicAdd((unsigned long long *)&info->mismatch, 1ull);
}

// ---- exclusive scan of int64 (tiles of 256 lanes x 8) ----
constexpr int kScanThreads = 256, kScanItems = 8, kScanTile = kScanThreads * kScanItems;

__global__ __launch_bounds__(kScanThreads) void scan_reduce_kernel(const long long *__restrict__ v, long long n, long long *__restrict__ partial)
{
  __shared__ long long waveSum[kScanThreads / 64];
  const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
  long long s = 0;
  for (int k = 0; k < kScanItems; k++) if (base + k < n) s += v[base + k];
  long long tot;
  gtxscan::tile_exclusive<kScanThreads>(s, waveSum, &tot);     // (only the block's sum is wanted)
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kScanThreads) void scan_partials_kernel(long long *__restrict__ partial, long long nt)
{
  __shared__ long long waveSum[kScanThreads / 64];
  gtxscan::run_exclusive_sum<kScanThreads>(partial, nt, partial, waveSum);
}

__global__ __launch_bounds__(kScanThreads) void scan_apply_kernel(long long *__restrict__ v, long long n, const long long *__restrict__ partial)
{
  __shared__ long long waveSum[kScanThreads / 64];
  const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
  long long x[kScanItems], s = 0;
  for (int k = 0; k < kScanItems; k++) { x[k] = base + k < n ? v[base + k] : 0; s += x[k]; }
  long long run = partial[blockIdx.x] + gtxscan::tile_exclusive<kScanThreads>(s, waveSum);
  for (int k = 0; k < kScanItems; k++) if (base + k < n) { v[base + k] = run; run += x[k]; }
}

__global__ void join_cut_kernel(const long long *__restrict__ off, long long q0, long long n, long long cap, long long *cut)
{
  const long long lim = off[q0] + cap;
  long long a = q0, b = n;                                    // off[a] <= lim; find the last such index in [q0, n]
  while (a < b) { const long long m = b - ((b - a) >> 1); if (off[m] <= lim) a = m; else b = m - 1; }
  *cut = a;
}

// ---- segment sort by (key[r], r) ----
__device__ __forceinline__ long long key_of(const long long *key, int r) { return key ? key[r] : (long long)r; }
__device__ __forceinline__ bool kr_less(long long ka, int ra, long long kb, int rb) { return ka < kb || (ka == kb && ra < rb); }

__global__ __launch_bounds__(256) void join_sort_small_kernel(const long long *__restrict__ off, long long q0, long long q1, const long long *__restrict__ key,
                                                              int *__restrict__ pairs, unsigned *__restrict__ big)
{
  const long long t = q0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= q1) return;
  const long long c = off[t + 1] - off[t];
  if (c < 2) return;
  if (c > kJoinSmallSeg) { const unsigned at = atomicAdd(big, 1u); big[1 + at] = (unsigned)(t - q0); return; }
  int *seg = pairs + (off[t] - off[q0]);
  for (int i = 1; i < (int)c; i++) {                          // insertion sort: segments arrive in start order, often nearly sorted
    const int r = seg[i]; const long long k = key_of(key, r);
    int j = i - 1;
    while (j >= 0) { const int y = seg[j]; if (!kr_less(k, r, key_of(key, y), y)) break; seg[j + 1] = y; j--; }
    seg[j + 1] = r;
  }
}

// bitonic sort of seg[0..c) (c <= kJoinLdsSeg) through LDS
__device__ void lds_sort(int *seg, int c, const long long *key, long long *sk, int *sr)
{
  int p = 1; while (p < c) p <<= 1;
  for (int i = threadIdx.x; i < p; i += blockDim.x) {
    if (i < c) { const int r = seg[i]; sr[i] = r; sk[i] = key_of(key, r); } else { sr[i] = INT_MAX; sk[i] = LLONG_MAX; }
  }
  __syncthreads();
  for (int k = 2; k <= p; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < p; i += blockDim.x) {
        const int x = i ^ j;
        if (x > i) {
          const bool up = (i & k) == 0;
          if (kr_less(sk[x], sr[x], sk[i], sr[i]) == up) {
            const long long tk = sk[i]; sk[i] = sk[x]; sk[x] = tk;
            const int tr = sr[i]; sr[i] = sr[x]; sr[x] = tr;
          }
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < c; i += blockDim.x) seg[i] = sr[i];
  __syncthreads();
}

// first index in run[0..n) whose (key, r) is not less than (k, r)
__device__ __forceinline__ int rank_in(const int *run, int n, long long k, int r, const long long *key)
{
  int a = 0, b = n;
  while (a < b) { const int m = (a + b) >> 1; const int y = run[m]; if (kr_less(key_of(key, y), y, k, r)) a = m + 1; else b = m; }
  return a;
}

__global__ __launch_bounds__(256) void join_sort_big_kernel(const long long *__restrict__ off, long long q0, const long long *__restrict__ key,
                                                            int *__restrict__ pairs, int *__restrict__ scratch, const unsigned *__restrict__ big)
{
  __shared__ long long sk[kJoinLdsSeg];
  __shared__ int sr[kJoinLdsSeg];
  const unsigned nBig = big[0];
  for (unsigned b = blockIdx.x; b < nBig; b += gridDim.x) {
    const long long t = q0 + big[1 + b];
    const long long o = off[t] - off[q0];
    const int c = (int)(off[t + 1] - off[t]);
    int *seg = pairs + o;
    for (int a0 = 0; a0 < c; a0 += kJoinLdsSeg) lds_sort(seg + a0, min(kJoinLdsSeg, c - a0), key, sk, sr);
    int *src = seg, *dst = scratch + o;
    for (long long w = kJoinLdsSeg; w < c; w <<= 1) {                // merge runs of w pairwise: a pair's place = its rank in its run + in the other
      for (int i = threadIdx.x; i < c; i += blockDim.x) {
        const long long a0l = (long long)(i / (2ll * w)) * (2ll * w);
        const int a0 = (int)a0l, mid = (int)min(a0l + w, (long long)c), end = (int)min(a0l + 2ll * w, (long long)c);
        const int r = src[i]; const long long k = key_of(key, r);
        const int pos = i < mid ? (i - a0) + rank_in(src + mid, end - mid, k, r, key) : (i - mid) + rank_in(src + a0, mid - a0, k, r, key);
        dst[a0 + pos] = r;
      }
      __syncthreads();
      int *tmp = src; src = dst; dst = tmp;
    }
    if (src != seg) { for (int i = threadIdx.x; i < c; i += blockDim.x) seg[i] = src[i]; }
    __syncthreads();
  }
}

inline unsigned grid_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_join_count(const JoinQueries &q, const PairIndex &ix, const RegionBlocks &rb, int mode, long long *off, JoinInfo *info, hipStream_t st)
{
  if (q.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(join_count_kernel, dim3(grid_of(q.n, 256)), dim3(256), 0, st, q, ix, rb, mode, off, info);
  return hipGetLastError();
}

long long join_scan_partials(long long n) { return (n + kScanTile - 1) / kScanTile + 1; }

hipError_t launch_join_scan(long long *v, long long n, long long *partial, hipStream_t st)
{
  if (n <= 0) return hipSuccess;
  const unsigned nt = grid_of(n, kScanTile);
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(nt), dim3(kScanThreads), 0, st, (const long long *)v, n, partial);
  hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, st, partial, (long long)nt);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(nt), dim3(kScanThreads), 0, st, v, n, (const long long *)partial);
  return hipGetLastError();
}

hipError_t launch_join_cut(const long long *off, long long q0, long long n, long long cap, long long *cut, hipStream_t st)
{
  hipLaunchKernelGGL(join_cut_kernel, dim3(1), dim3(1), 0, st, off, q0, n, cap, cut);
  return hipGetLastError();
}

hipError_t launch_join_emit(const JoinQueries &q, long long q0, long long q1, const PairIndex &ix, const RegionBlocks &rb, int mode,
                            const long long *off, int *pairs, JoinInfo *info, hipStream_t st)
{
  if (q1 <= q0) return hipSuccess;
  hipLaunchKernelGGL(join_emit_kernel, dim3(grid_of(q1 - q0, 256)), dim3(256), 0, st, q, q0, q1, ix, rb, mode, off, pairs, info);
  return hipGetLastError();
}

hipError_t launch_join_sort(const long long *off, long long q0, long long q1, const long long *key, int *pairs, int *scratch, unsigned *big, hipStream_t st)
{
  if (q1 <= q0) return hipSuccess;
  hipError_t e = hipMemsetAsync(big, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(join_sort_small_kernel, dim3(grid_of(q1 - q0, 256)), dim3(256), 0, st, off, q0, q1, key, pairs, big);
  hipLaunchKernelGGL(join_sort_big_kernel, dim3(1024), dim3(256), 0, st, off, q0, key, pairs, scratch, (const unsigned *)big);
  return hipGetLastError();
}

}  // namespace gtx
