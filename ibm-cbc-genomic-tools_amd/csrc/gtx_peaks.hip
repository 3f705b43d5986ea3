// Kernels of the peak candidate selection (see gtx_peaks.h).  A tile is kPeakTile windows and belongs to one wave: kPeakRows rows of
// 128 consecutive windows, lane l of a row reading windows 2 l and 2 l + 1 of every vector with one 16-byte load.  The rank of a kept
// window inside its tile is the wave-uniform count of the rows in front of it plus the popcounts of the row's two ballots below its
// lane (gtx_select.hip).
#include "gtx_peaks.h"
#include "gtx_select.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr int kWaves = kPeakThreads / 64;

// windows i and i + 1 of a vector (i even, the vector 16-byte aligned); what lies behind the end reads as 0
__device__ __forceinline__ u64x2 load_pair(const u64 *__restrict__ p, i64 i, i64 n)
{
  if (i + 1 < n) return __builtin_nontemporal_load((const u64x2 *)(p + i));
  u64x2 v; v.x = i < n ? __builtin_nontemporal_load(p + i) : 0ull; v.y = 0ull;
  return v;
}

// one window's three counts after clamp and norm (genomic_scans.cpp:304-311)
struct Row { i64 v1, v2, v0; };

__device__ __forceinline__ Row peak_row(u64 s, u64 c, i64 v0, int norm, double ratio)
{
  Row r;
  r.v0 = v0;
  r.v1 = min((i64)s, v0);
  r.v2 = min((i64)c, v0);
  if (norm == 1) r.v2 = (i64)floor((double)(float)r.v2 * ratio);
  else if (norm == 2) r.v1 = (i64)floor((double)(float)r.v1 / ratio);
  return r;
}

// EMIT = false: the tile's number of kept windows.  EMIT = true: the kept windows' ordinals and rows at tileBase[tile] + rank.
template <bool UNIQ, bool EMIT>
__global__ __launch_bounds__(kPeakThreads) void peak_kernel(PeakArgs a, i64 nt, unsigned *__restrict__ tileCount, const i64 *__restrict__ tileBase, i64 capacity,
                                                            i64 *__restrict__ ordinals, i64 *__restrict__ rows)
{
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 t = (i64)blockIdx.x * kWaves + w;
  if (t >= nt) return;
  i64 base = 0;
  if (EMIT) {
    base = tileBase[t];
    if (tileBase[t + 1] == base || base >= capacity) return;         // nothing kept here (the tile is not loaded), or everything behind the caller's room
  }
  const i64 tileStart = t * kPeakTile;
  unsigned before = 0;                                                // kept in the rows in front (wave-uniform)
#pragma unroll 2
  for (int r = 0; r < kPeakRows; r++) {
    if (tileStart + (i64)r * 128 >= a.n) break;
    const i64 i = tileStart + (i64)r * 128 + 2 * lane;
    const u64x2 s = load_pair(a.signal, i, a.n), c = load_pair(a.control, i, a.n);
    i64 u0 = a.winSize, u1 = a.winSize;
    if (UNIQ) { const u64x2 u = load_pair(a.uniq, i, a.n); u0 = (i64)u.x; u1 = (i64)u.y; }
    const Row r0 = peak_row(s.x, c.x, u0, a.norm, a.ratio), r1 = peak_row(s.y, c.y, u1, a.norm, a.ratio);
    const bool keep0 = i < a.n && r0.v1 >= a.minReads, keep1 = i + 1 < a.n && r1.v1 >= a.minReads;
    const u64 b0 = __ballot(keep0), b1 = __ballot(keep1);
    if (EMIT) {
      const u64 below = (1ull << lane) - 1;
      const i64 g0 = base + before + __popcll(b0 & below) + __popcll(b1 & below), g1 = g0 + (keep0 ? 1 : 0);
      if (keep0 && g0 < capacity) { ordinals[g0] = i; rows[3 * g0] = r0.v1; rows[3 * g0 + 1] = r0.v2; rows[3 * g0 + 2] = r0.v0; }
      if (keep1 && g1 < capacity) { ordinals[g1] = i + 1; rows[3 * g1] = r1.v1; rows[3 * g1 + 1] = r1.v2; rows[3 * g1 + 2] = r1.v0; }
    }
    before += (unsigned)(__popcll(b0) + __popcll(b1));
  }
  if (!EMIT && lane == 0) tileCount[t] = before;
}

template <bool UNIQ>
hipError_t launch_passes(const PeakArgs &a, i64 nt, unsigned *tileCount, i64 *tileBase, i64 capacity, i64 *ordinals, i64 *rows, hipStream_t st)
{
  const unsigned grid = (unsigned)((nt + kWaves - 1) / kWaves);
  hipLaunchKernelGGL((peak_kernel<UNIQ, false>), dim3(grid), dim3(kPeakThreads), 0, st, a, nt, tileCount, (const i64 *)nullptr, capacity, (i64 *)nullptr,
                     (i64 *)nullptr);
  const hipError_t e = launch_tile_prefix(tileCount, nt, tileBase, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((peak_kernel<UNIQ, true>), dim3(grid), dim3(kPeakThreads), 0, st, a, nt, (unsigned *)nullptr, (const i64 *)tileBase, capacity, ordinals, rows);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_peak_select(const PeakArgs &a, unsigned *tileCount, long long *tileBase, long long capacity, long long *ordinals, long long *rows,
                              hipStream_t st)
{
  const i64 nt = peak_tiles(a.n);
  return a.uniq ? launch_passes<true>(a, nt, tileCount, tileBase, capacity, ordinals, rows, st)
                : launch_passes<false>(a, nt, tileCount, tileBase, capacity, ordinals, rows, st);
}

}  // namespace gtx
