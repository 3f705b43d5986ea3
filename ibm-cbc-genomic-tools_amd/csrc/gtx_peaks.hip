// Kernels of the peak candidate selection (see gtx_peaks.h): the rule of the tile compaction (gtx_compact.h, which has the shape of the
// passes) and its dispatch.
#include "gtx_peaks.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;

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

// A window is kept when its v1 reaches min_reads; its row is v1, v2, v0.
template <bool UNIQ>
struct PeakRule : CompactRule {
  PeakArgs a;
  typedef Row Payload;

  __device__ __forceinline__ void load(i64 i, i64 n, Row &p0, Row &p1) const
  {
    const u64x2 s = load_pair(a.signal, i, n), c = load_pair(a.control, i, n);
    i64 u0 = a.winSize, u1 = a.winSize;
    if (UNIQ) { const u64x2 u = load_pair(a.uniq, i, n); u0 = (i64)u.x; u1 = (i64)u.y; }
    p0 = peak_row(s.x, c.x, u0, a.norm, a.ratio); p1 = peak_row(s.y, c.y, u1, a.norm, a.ratio);
  }
  __device__ __forceinline__ bool keep(i64, const Row &p) const { return p.v1 >= a.minReads; }
  __device__ __forceinline__ void emit(i64 *__restrict__ rows, i64 g, i64, const Row &p) const { rows[3 * g] = p.v1; rows[3 * g + 1] = p.v2; rows[3 * g + 2] = p.v0; }
};

template <bool UNIQ>
hipError_t launch_rule(const PeakArgs &a, unsigned *tileCount, i64 *tileBase, i64 capacity, i64 *ordinals, i64 *rows, hipStream_t st)
{
  PeakRule<UNIQ> rule; rule.a = a;
  return launch_compact(rule, a.n, tileCount, tileBase, capacity, ordinals, rows, st);
}

}  // namespace

hipError_t launch_peak_select(const PeakArgs &a, unsigned *tileCount, long long *tileBase, long long capacity, long long *ordinals, long long *rows,
                              hipStream_t st)
{
  return a.uniq ? launch_rule<true>(a, tileCount, tileBase, capacity, ordinals, rows, st) : launch_rule<false>(a, tileCount, tileBase, capacity, ordinals, rows, st);
}

}  // namespace gtx
