// Kernels of the window selection (see gtx_select.h).  A tile is kSelectTile windows and belongs to one wave: kSelectRows rows of
// 128 consecutive windows, lane l of a row reading windows 2 l and 2 l + 1 of every vector with one 16-byte load.  The rank of a kept
// window inside its tile is the wave-uniform count of the rows in front of it plus the popcounts of the row's two ballots below its
// lane, so the waves of a block share nothing but the tables.
#include "gtx_select.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr int kWaves = kSelectThreads / 64;

// windows i and i + 1 of a vector (i even, the vector 16-byte aligned); what lies behind the end reads as 0
__device__ __forceinline__ u64x2 load_pair(const u64 *__restrict__ p, i64 i, i64 n)
{
  if (i + 1 < n) return __builtin_nontemporal_load((const u64x2 *)(p + i));
  u64x2 v; v.x = i < n ? __builtin_nontemporal_load(p + i) : 0ull; v.y = 0ull;
  return v;
}

// EMIT = false: the tile's number of kept windows.  EMIT = true: the kept windows' ordinals and rows at tileBase[tile] + rank.
template <int NT, bool CTL, bool LDS, bool EMIT>
__global__ __launch_bounds__(kSelectThreads) void select_kernel(SelectArgs a, i64 nt, unsigned *__restrict__ tileCount, const i64 *__restrict__ tileBase,
                                                                i64 capacity, i64 *__restrict__ ordinals, int *__restrict__ rows)
{
  extern __shared__ int shTab[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int stride = CTL ? a.W + 1 : 1;
  if (LDS) {
    for (int j = threadIdx.x; j < NT * stride; j += kSelectThreads) shTab[j] = a.tab[j];
    __syncthreads();
  }
  const i64 t = (i64)blockIdx.x * kWaves + w;
  if (t >= nt) return;
  i64 base = 0;
  if (EMIT) {
    base = tileBase[t];
    if (tileBase[t + 1] == base || base >= capacity) return;         // nothing kept here, or everything behind the caller's room
  }
  const u64 W = (u64)a.W;
  const i64 tileStart = t * kSelectTile;
  constexpr int kCols = CTL ? 2 * NT : NT;
  unsigned before = 0;                                                // kept in the rows in front (wave-uniform)
#pragma unroll 2
  for (int r = 0; r < kSelectRows; r++) {
    const i64 i = tileStart + (i64)r * 128 + 2 * lane;
    int k[NT][2], c[NT][2];
    bool keep0 = false, keep1 = false;
#pragma unroll
    for (int f = 0; f < NT; f++) {
      const u64x2 v = load_pair(a.tested[f], i, a.n);
      k[f][0] = (int)(v.x < W ? v.x : W); k[f][1] = (int)(v.y < W ? v.y : W);
      c[f][0] = 0; c[f][1] = 0;
      if (CTL) {
        const u64x2 q = load_pair(a.control[f], i, a.n);
        c[f][0] = (int)(q.x < W ? q.x : W); c[f][1] = (int)(q.y < W ? q.y : W);
      }
      const int crit0 = LDS ? shTab[f * stride + c[f][0]] : a.tab[f * stride + c[f][0]];
      const int crit1 = LDS ? shTab[f * stride + c[f][1]] : a.tab[f * stride + c[f][1]];
      keep0 |= k[f][0] >= crit0; keep1 |= k[f][1] >= crit1;
    }
    keep0 &= i < a.n; keep1 &= i + 1 < a.n;
    const u64 b0 = __ballot(keep0), b1 = __ballot(keep1);
    if (EMIT) {
      const u64 below = (1ull << lane) - 1;
      const i64 g0 = base + before + __popcll(b0 & below) + __popcll(b1 & below), g1 = g0 + (keep0 ? 1 : 0);
      if (keep0 && g0 < capacity) {
        ordinals[g0] = i;
#pragma unroll
        for (int f = 0; f < NT; f++) { rows[g0 * kCols + f] = k[f][0]; if (CTL) rows[g0 * kCols + NT + f] = c[f][0]; }
      }
      if (keep1 && g1 < capacity) {
        ordinals[g1] = i + 1;
#pragma unroll
        for (int f = 0; f < NT; f++) { rows[g1 * kCols + f] = k[f][1]; if (CTL) rows[g1 * kCols + NT + f] = c[f][1]; }
      }
    }
    before += (unsigned)(__popcll(b0) + __popcll(b1));
  }
  if (!EMIT && lane == 0) tileCount[t] = before;
}

// exclusive sum of the tiles' counts in one block, each lane over a run of consecutive tiles with its loads out eight at a time
// (gtx_link.hip: link_heads_kernel); base[nt] = the number kept
constexpr int kPartThreads = 1024, kPartBatch = 8;
__global__ __launch_bounds__(kPartThreads) void select_prefix_kernel(const unsigned *__restrict__ count, i64 nt, i64 *__restrict__ base)
{
  __shared__ i64 sh[kPartThreads];
  const int tid = threadIdx.x;
  const i64 per = (nt + kPartThreads - 1) / kPartThreads, b = min((i64)tid * per, nt), e = min(b + per, nt);
  i64 a = 0;
  for (i64 k = b; k < e; k += kPartBatch) {
    unsigned v[kPartBatch];
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) v[j] = k + j < e ? count[k + j] : 0u;
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) a += v[j];
  }
  sh[tid] = a;
  __syncthreads();
  for (int dd = 1; dd < kPartThreads; dd <<= 1) {
    const i64 o = tid >= dd ? sh[tid - dd] : 0;
    __syncthreads();
    sh[tid] += o;
    __syncthreads();
  }
  i64 run = tid > 0 ? sh[tid - 1] : 0;
  for (i64 k = b; k < e; k += kPartBatch) {
    unsigned v[kPartBatch];
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) v[j] = k + j < e ? count[k + j] : 0u;
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) if (k + j < e) { base[k + j] = run; run += v[j]; }
  }
  if (tid == kPartThreads - 1) base[nt] = sh[tid];
}

template <int NT, bool CTL, bool LDS>
void launch_passes(const SelectArgs &a, i64 nt, unsigned *tileCount, i64 *tileBase, i64 capacity, i64 *ordinals, int *rows, hipStream_t st)
{
  const unsigned grid = (unsigned)((nt + kWaves - 1) / kWaves);
  const size_t lds = LDS ? (size_t)NT * (CTL ? a.W + 1 : 1) * sizeof(int) : 0;
  hipLaunchKernelGGL((select_kernel<NT, CTL, LDS, false>), dim3(grid), dim3(kSelectThreads), lds, st, a, nt, tileCount, (const i64 *)nullptr, capacity,
                     (i64 *)nullptr, (int *)nullptr);
  hipLaunchKernelGGL(select_prefix_kernel, dim3(1), dim3(kPartThreads), 0, st, (const unsigned *)tileCount, nt, tileBase);
  hipLaunchKernelGGL((select_kernel<NT, CTL, LDS, true>), dim3(grid), dim3(kSelectThreads), lds, st, a, nt, (unsigned *)nullptr, (const i64 *)tileBase, capacity,
                     ordinals, rows);
}

template <int NT>
void launch_tested(const SelectArgs &a, bool ctl, bool lds, i64 nt, unsigned *tileCount, i64 *tileBase, i64 capacity, i64 *ordinals, int *rows, hipStream_t st)
{
  if (ctl) { if (lds) launch_passes<NT, true, true>(a, nt, tileCount, tileBase, capacity, ordinals, rows, st); else launch_passes<NT, true, false>(a, nt, tileCount, tileBase, capacity, ordinals, rows, st); }
  else { if (lds) launch_passes<NT, false, true>(a, nt, tileCount, tileBase, capacity, ordinals, rows, st); else launch_passes<NT, false, false>(a, nt, tileCount, tileBase, capacity, ordinals, rows, st); }
}

}  // namespace

hipError_t launch_tile_prefix(const unsigned *tileCount, long long tiles, long long *tileBase, hipStream_t st)
{
  hipLaunchKernelGGL(select_prefix_kernel, dim3(1), dim3(kPartThreads), 0, st, tileCount, tiles, tileBase);
  return hipGetLastError();
}

hipError_t launch_window_select(const SelectArgs &a, unsigned *tileCount, long long *tileBase, long long capacity, long long *ordinals, int *rows,
                                hipStream_t st)
{
  const i64 nt = select_tiles(a.n);
  const bool ctl = a.control[0] != nullptr, lds = select_tables_in_lds(a.nTested, a.W, ctl);
  switch (a.nTested) {
    case 1: launch_tested<1>(a, ctl, lds, nt, tileCount, tileBase, capacity, ordinals, rows, st); break;
    case 2: launch_tested<2>(a, ctl, lds, nt, tileCount, tileBase, capacity, ordinals, rows, st); break;
    case 3: launch_tested<3>(a, ctl, lds, nt, tileCount, tileBase, capacity, ordinals, rows, st); break;
    case 4: launch_tested<4>(a, ctl, lds, nt, tileCount, tileBase, capacity, ordinals, rows, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace gtx
