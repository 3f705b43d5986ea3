// Kernels of the window selection (see gtx_select.h): the rule of the tile compaction (gtx_compact.h, which has the shape of the
// passes) and its dispatch, and the tile prefix every user of that shape launches.
#include "gtx_select.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;

// A window is kept when k_f >= kcrit_f[c_f] for any tested vector f, k and c the vector's and its control's sums clamped to W; its row
// is the k_f, then the c_f.  The tables are read from LDS (a block copies them there first) or from global memory.
template <int NT, bool CTL, bool LDS>
struct SelectRule : CompactRule {
  SelectArgs a;
  struct Payload { int k[NT], c[NT]; bool hit; };                     // hit: some k_f has reached its critical count
  static constexpr int kCols = CTL ? 2 * NT : NT;
  static constexpr bool kTwoRowsInFlight = true;

  size_t lds_bytes() const { return LDS ? (size_t)NT * (CTL ? a.W + 1 : 1) * sizeof(int) : 0; }
  __device__ __forceinline__ void block()
  {
    extern __shared__ int shTab[];
    if (LDS) {
      for (int j = threadIdx.x; j < NT * (CTL ? a.W + 1 : 1); j += kCompactThreads) shTab[j] = a.tab[j];
      __syncthreads();
    }
  }
  // (the tables are looked up as the counts arrive, vector by vector: the loaded sums do not stay live)
  __device__ __forceinline__ void load(i64 i, i64 n, Payload &p0, Payload &p1) const
  {
    extern __shared__ int shTab[];
    const u64 W = (u64)a.W;
    const int stride = CTL ? a.W + 1 : 1;
    p0.hit = false; p1.hit = false;
#pragma unroll
    for (int f = 0; f < NT; f++) {
      const u64x2 v = load_pair(a.tested[f], i, n);
      p0.k[f] = (int)(v.x < W ? v.x : W); p1.k[f] = (int)(v.y < W ? v.y : W);
      p0.c[f] = 0; p1.c[f] = 0;
      if (CTL) {
        const u64x2 q = load_pair(a.control[f], i, n);
        p0.c[f] = (int)(q.x < W ? q.x : W); p1.c[f] = (int)(q.y < W ? q.y : W);
      }
      const int crit0 = LDS ? shTab[f * stride + p0.c[f]] : a.tab[f * stride + p0.c[f]];
      const int crit1 = LDS ? shTab[f * stride + p1.c[f]] : a.tab[f * stride + p1.c[f]];
      p0.hit |= p0.k[f] >= crit0; p1.hit |= p1.k[f] >= crit1;
    }
  }
  __device__ __forceinline__ bool keep(i64, const Payload &p) const { return p.hit; }
  __device__ __forceinline__ void emit(int *__restrict__ rows, i64 g, i64, const Payload &p) const
  {
#pragma unroll
    for (int f = 0; f < NT; f++) { rows[g * kCols + f] = p.k[f]; if (CTL) rows[g * kCols + NT + f] = p.c[f]; }
  }
};

template <class COUNT>
__global__ __launch_bounds__(kPartThreads) void select_prefix_kernel(const COUNT *__restrict__ count, i64 nt, i64 *__restrict__ base)
{
  __shared__ i64 sh[kPartThreads];
  block_exclusive_sum(count, nt, base, sh);
}

template <int NT, bool CTL, bool LDS>
hipError_t launch_rule(const SelectArgs &a, unsigned *tileCount, i64 *tileBase, i64 capacity, i64 *ordinals, int *rows, hipStream_t st)
{
  SelectRule<NT, CTL, LDS> rule; rule.a = a;
  return launch_compact(rule, a.n, tileCount, tileBase, capacity, ordinals, rows, st);
}

template <int NT>
hipError_t launch_tested(const SelectArgs &a, bool ctl, bool lds, unsigned *tileCount, i64 *tileBase, i64 capacity, i64 *ordinals, int *rows, hipStream_t st)
{
  if (ctl) return lds ? launch_rule<NT, true, true>(a, tileCount, tileBase, capacity, ordinals, rows, st) : launch_rule<NT, true, false>(a, tileCount, tileBase, capacity, ordinals, rows, st);
  return lds ? launch_rule<NT, false, true>(a, tileCount, tileBase, capacity, ordinals, rows, st) : launch_rule<NT, false, false>(a, tileCount, tileBase, capacity, ordinals, rows, st);
}

}  // namespace

hipError_t launch_tile_prefix(const unsigned *tileCount, long long tiles, long long *tileBase, hipStream_t st)
{
  hipLaunchKernelGGL(select_prefix_kernel<unsigned>, dim3(1), dim3(kPartThreads), 0, st, tileCount, tiles, tileBase);
  return hipGetLastError();
}

hipError_t launch_tile_prefix64(const unsigned long long *tileCount, long long tiles, long long *tileBase, hipStream_t st)
{
  hipLaunchKernelGGL(select_prefix_kernel<unsigned long long>, dim3(1), dim3(kPartThreads), 0, st, tileCount, tiles, tileBase);
  return hipGetLastError();
}

hipError_t launch_window_select(const SelectArgs &a, unsigned *tileCount, long long *tileBase, long long capacity, long long *ordinals, int *rows,
                                hipStream_t st)
{
  const bool ctl = a.control[0] != nullptr, lds = select_tables_in_lds(a.nTested, a.W, ctl);
  switch (a.nTested) {
    case 1: return launch_tested<1>(a, ctl, lds, tileCount, tileBase, capacity, ordinals, rows, st);
    case 2: return launch_tested<2>(a, ctl, lds, tileCount, tileBase, capacity, ordinals, rows, st);
    case 3: return launch_tested<3>(a, ctl, lds, tileCount, tileBase, capacity, ordinals, rows, st);
    case 4: return launch_tested<4>(a, ctl, lds, tileCount, tileBase, capacity, ordinals, rows, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace gtx
