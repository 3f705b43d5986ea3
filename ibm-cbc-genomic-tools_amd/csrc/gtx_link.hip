// Kernels of link (see gtx_link.h).  A tile is kLinkTile regions: four waves, each over a span of 8 rows of 64 consecutive regions,
// lane l of a row reading region row * 64 + l -- the 12-bytes-per-lane non-temporal load pattern of the streaming count kernel
// (gtx_kernels.hip: load_tri).  Scans run along a row with wave shuffles, from row to row and wave to wave through wave-uniform
// carries.
#include <climits>
#include "gtx_link.h"
#include "gtx_compact.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kSpan = 64 * kLinkRows;          // regions per wave
constexpr int kWaves = kLinkThreads / 64;

// element of the class-segmented maximum: f = a class break at or in front of here, m = the largest stop since the last break
struct SegMax { int f, m; };
__device__ __forceinline__ SegMax seg_comb(SegMax a, SegMax b) { SegMax r; r.f = a.f | b.f; r.m = b.f ? b.m : max(a.m, b.m); return r; }
__device__ __forceinline__ SegMax seg_identity() { SegMax r; r.f = 0; r.m = INT_MIN; return r; }

// APPLY = false: the tile's aggregate and the order check.  APPLY = true: with the tiles' exclusive prefixes, the break flag of every
// region -- first of its class, or START - P > d in 64 bits, P the class's largest stop in front of it -- and the tile's heads.
template <bool APPLY>
__global__ __launch_bounds__(kLinkThreads) void link_scan_kernel(const int *__restrict__ tri, i64 n, i64 d, const int2 *__restrict__ tilePrefix,
                                                                 int2 *__restrict__ tileAgg, u64 *__restrict__ firstUnsorted, u64 *__restrict__ bits,
                                                                 unsigned *__restrict__ tileHeads)
{
  __shared__ int2 shAgg[kWaves];
  __shared__ unsigned shHeads[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 tileBase = (i64)blockIdx.x * kLinkTile, spanBase = tileBase + (i64)w * kSpan;
  int prevC = 0, prevS = 0;                                           // the region in front of the span (wave-uniform)
  if (spanBase > 0 && spanBase < n) { prevC = tri[3 * (spanBase - 1)]; prevS = tri[3 * (spanBase - 1) + 1]; }
  int c[kLinkRows], s[kLinkRows], e[kLinkRows];
#pragma unroll
  for (int k = 0; k < kLinkRows; k++) {
    const i64 i = spanBase + 64 * k + lane;
    c[k] = 0; s[k] = 0; e[k] = INT_MIN;
    if (i < n) { c[k] = __builtin_nontemporal_load(tri + 3 * i); s[k] = __builtin_nontemporal_load(tri + 3 * i + 1); e[k] = __builtin_nontemporal_load(tri + 3 * i + 2); }
  }
  unsigned breakBits = 0;
  if (!APPLY) {
    // the span's aggregate without a scan: where its last class break is (a ballot per row), then one wave maximum over the stops
    // behind it; the order check rides on the same predecessor values
    i64 unsortedAt = -1;
    int lastRow = -1, lastLane = 0;
#pragma unroll
    for (int k = 0; k < kLinkRows; k++) {
      const i64 i = spanBase + 64 * k + lane;
      const bool valid = i < n;
      int pc = __shfl_up(c[k], 1), ps = __shfl_up(s[k], 1);
      const int lc = k ? __shfl(c[k ? k - 1 : 0], 63) : prevC, ls = k ? __shfl(s[k ? k - 1 : 0], 63) : prevS;
      if (lane == 0) { pc = lc; ps = ls; }
      const u64 bb = __ballot(valid && (i == 0 || c[k] != pc));
      if (bb) { lastRow = k; lastLane = 63 - __builtin_clzll(bb); }
      const u64 ub = __ballot(valid && i > 0 && (c[k] < pc || (c[k] == pc && s[k] < ps)));
      if (ub && unsortedAt < 0) unsortedAt = spanBase + 64 * k + __builtin_ctzll(ub);
    }
    int m = INT_MIN;
#pragma unroll
    for (int k = 0; k < kLinkRows; k++) if (k > lastRow || (k == lastRow && lane >= lastLane)) m = max(m, e[k]);
#pragma unroll
    for (int dd = 32; dd > 0; dd >>= 1) m = max(m, __shfl_xor(m, dd));
    if (lane == 0) {
      shAgg[w] = make_int2(lastRow >= 0, m);
      if (unsortedAt >= 0) atomicMin(firstUnsorted, (u64)unsortedAt);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      SegMax t; t.f = shAgg[0].x; t.m = shAgg[0].y;
      for (int j = 1; j < kWaves; j++) { SegMax o; o.f = shAgg[j].x; o.m = shAgg[j].y; t = seg_comb(t, o); }
      tileAgg[blockIdx.x] = make_int2(t.f, t.m);
    }
    return;
  }
  int inF[kLinkRows], inM[kLinkRows];                                 // inclusive scan along each row
  SegMax rowAgg[kLinkRows];
#pragma unroll
  for (int k = 0; k < kLinkRows; k++) {
    const i64 i = spanBase + 64 * k + lane;
    const bool valid = i < n;
    int pc = __shfl_up(c[k], 1);
    const int lc = k ? __shfl(c[k ? k - 1 : 0], 63) : prevC;
    if (lane == 0) pc = lc;
    const bool brk = valid && (i == 0 || c[k] != pc);
    breakBits |= (unsigned)brk << k;
    int F = brk, M = e[k];
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
      const int oF = __shfl_up(F, dd), oM = __shfl_up(M, dd);
      if (lane >= dd) { M = F ? M : max(oM, M); F |= oF; }
    }
    inF[k] = F; inM[k] = M;
    rowAgg[k].f = __shfl(F, 63); rowAgg[k].m = __shfl(M, 63);
  }
  SegMax agg = rowAgg[0];
#pragma unroll
  for (int k = 1; k < kLinkRows; k++) agg = seg_comb(agg, rowAgg[k]);
  if (lane == 0) shAgg[w] = make_int2(agg.f, agg.m);
  __syncthreads();
  SegMax carry; { const int2 p = tilePrefix[blockIdx.x]; carry.f = p.x; carry.m = p.y; }
  for (int j = 0; j < w; j++) { SegMax o; o.f = shAgg[j].x; o.m = shAgg[j].y; carry = seg_comb(carry, o); }
  unsigned heads = 0;
#pragma unroll
  for (int k = 0; k < kLinkRows; k++) {
    const i64 i = spanBase + 64 * k + lane;
    SegMax ex; ex.f = __shfl_up(inF[k], 1); ex.m = __shfl_up(inM[k], 1);
    if (lane == 0) ex = seg_identity();
    const SegMax p = seg_comb(carry, ex);                             // everything in front of region i
    const bool brk = (breakBits >> k) & 1;
    const bool head = i < n && (brk || (i64)s[k] - (i64)p.m > d);
    const u64 word = __ballot(head);
    if (lane == 0) bits[(spanBase + 64 * k) >> 6] = word;
    heads += (unsigned)__popcll(word);
    carry = seg_comb(carry, rowAgg[k]);
  }
  if (lane == 0) shHeads[w] = heads;
  __syncthreads();
  if (threadIdx.x == 0) { unsigned t = 0; for (int j = 0; j < kWaves; j++) t += shHeads[j]; tileHeads[blockIdx.x] = t; }
}

// The two scans over per-tile values run in one block of kPartThreads lanes, each over a run of consecutive tiles with its loads out
// kPartBatch at a time, the runs' summaries joined by tile_exclusive (gtx_scan.h).
struct SegComb { __device__ __forceinline__ SegMax operator()(SegMax a, SegMax b) const { return seg_comb(a, b); } };

// exclusive scan of the tiles' aggregates
__global__ __launch_bounds__(kPartThreads) void link_prefix_kernel(const int2 *__restrict__ agg, i64 nt, int2 *__restrict__ prefix)
{
  __shared__ SegMax waveAgg[kPartThreads / 64];
  const int tid = threadIdx.x;
  const i64 per = (nt + kPartThreads - 1) / kPartThreads, b = min((i64)tid * per, nt), e = min(b + per, nt);
  SegMax a = seg_identity();
  for (i64 k = b; k < e; k += kPartBatch) {
    int2 v[kPartBatch];
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) v[j] = k + j < e ? agg[k + j] : make_int2(0, INT_MIN);
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) { SegMax o; o.f = v[j].x; o.m = v[j].y; a = seg_comb(a, o); }
  }
  SegMax run = gtxscan::tile_exclusive<kPartThreads>(a, waveAgg, (SegMax *)nullptr, seg_identity(), SegComb());
  for (i64 k = b; k < e; k += kPartBatch) {
    int2 v[kPartBatch];
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) v[j] = k + j < e ? agg[k + j] : make_int2(0, INT_MIN);
#pragma unroll
    for (int j = 0; j < kPartBatch; j++) if (k + j < e) { SegMax o; o.f = v[j].x; o.m = v[j].y; prefix[k + j] = make_int2(run.f, run.m); run = seg_comb(run, o); }
  }
}

// exclusive sum of the tiles' heads (base[nt] = all heads), then the groups that count: with no unsorted region all of them; else those
// closed in front of the first unsorted region U, i.e. the heads in [0, U) less the one whose group is open at U
__global__ __launch_bounds__(kPartThreads) void link_heads_kernel(const unsigned *__restrict__ heads, i64 nt, i64 *__restrict__ base,
                                                                  const u64 *__restrict__ bits, LinkInfo *info)
{
  __shared__ i64 sh[kPartThreads];
  block_exclusive_sum(heads, nt, base, sh);
  if (threadIdx.x == 0) {
    const u64 U = info->firstUnsorted;
    if (U == ~0ull) { info->nGroups = base[nt]; info->firstUnsortedOut = -1; }
    else {
      const i64 t = (i64)(U / kLinkTile);
      i64 h = base[t];
      for (i64 wd = t * (kLinkTile / 64); wd <= (i64)(U >> 6); wd++) {
        u64 m = bits[wd];
        if (wd == (i64)(U >> 6)) m &= (1ull << (U & 63)) - 1;
        h += __popcll(m);
      }
      info->nGroups = h - 1;
      info->firstUnsortedOut = (i64)U;
    }
  }
}

// ---- the groups' records ----
struct Part { unsigned cnt; int mx; i64 v; };

template <int MODE> __device__ __forceinline__ i64 val_identity() { return MODE == LINK_MIN ? LLONG_MAX : MODE == LINK_MAX ? LLONG_MIN : 0; }
template <int MODE> __device__ __forceinline__ i64 val_comb(i64 a, i64 b)
{
  return MODE == LINK_SUM ? (i64)((u64)a + (u64)b) : MODE == LINK_MIN ? min(a, b) : MODE == LINK_MAX ? max(a, b) : 0;
}
template <int MODE> __device__ __forceinline__ Part part_identity() { Part p; p.cnt = 0; p.mx = INT_MIN; p.v = val_identity<MODE>(); return p; }
template <int MODE> __device__ __forceinline__ Part part_comb(Part a, Part b) { Part r; r.cnt = a.cnt + b.cnt; r.mx = max(a.mx, b.mx); r.v = val_comb<MODE>(a.v, b.v); return r; }

template <int MODE> __device__ __forceinline__ void put_whole(i64 g, i64 nGroups, Part p, unsigned *cnt, int *stop, i64 *val)
{
  if (g < 0 || g >= nGroups) return;
  cnt[g] = p.cnt; stop[g] = p.mx;
  if (MODE != LINK_NONE) val[g] = p.v;
}
template <int MODE> __device__ __forceinline__ void put_piece(i64 g, i64 nGroups, Part p, unsigned *cnt, int *stop, i64 *val)
{
  if (g < 0 || g >= nGroups) return;
  atomicAdd(cnt + g, p.cnt); atomicMax(stop + g, p.mx);
  if (MODE == LINK_SUM) atomicAdd((u64 *)(val + g), (u64)p.v);
  if (MODE == LINK_MIN) atomicMin(val + g, p.v);
  if (MODE == LINK_MAX) atomicMax(val + g, p.v);
}

// a group that reaches over the front of tile t (its first region is no head) gets its pieces by atomics: the identity first
template <int MODE>
__global__ __launch_bounds__(256) void link_init_kernel(const u64 *__restrict__ bits, const i64 *__restrict__ base, i64 nt, const LinkInfo *info,
                                                        unsigned *__restrict__ cnt, int *__restrict__ stop, i64 *__restrict__ val)
{
  const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 1 || t >= nt || (bits[t * (kLinkTile / 64)] & 1)) return;
  const i64 g = base[t] - 1;
  if (g < 0 || g >= info->nGroups) return;
  cnt[g] = 0; stop[g] = INT_MIN;
  if (MODE != LINK_NONE) val[g] = val_identity<MODE>();
}

template <int MODE>
__global__ __launch_bounds__(kLinkThreads) void link_groups_kernel(const int *__restrict__ tri, const i64 *__restrict__ vals, i64 n, const u64 *__restrict__ bits,
                                                                   const i64 *__restrict__ base, const LinkInfo *info, unsigned *__restrict__ headOut,
                                                                   unsigned *__restrict__ cntOut, int *__restrict__ stopOut, i64 *__restrict__ valOut)
{
  // per wave: A = the regions in front of the span's first group end (they continue the group that reaches into the span), closed =
  // such an end exists; B = the group open at the span's end (hasB)
  __shared__ Part shA[kWaves], shB[kWaves];
  __shared__ int shClosed[kWaves], shHasB[kWaves];
  __shared__ i64 shGB[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 t = blockIdx.x, tileBase = t * kLinkTile, spanBase = tileBase + (i64)w * kSpan;
  const i64 nGroups = info->nGroups, tb = base[t];
  // heads in front of every row of the tile
  const u64 myWord = lane < kLinkTile / 64 ? bits[t * (kLinkTile / 64) + lane] : 0;
  const int own = __popcll(myWord), incl = gtxscan::wave_inclusive(own), excl = incl - own;
  Part carry = part_identity<MODE>();
  bool leftOpen = true, dead = false;
#pragma unroll
  for (int k = 0; k < kLinkRows; k++) {
    const int wi = w * kLinkRows + k;
    const u64 H = __shfl(myWord, wi);
    const i64 rowBase = tb + __shfl(excl, wi);
    const i64 i0 = spanBase + 64 * k, i = i0 + lane;
    const u64 V = i0 >= n ? 0ull : (n - i0 >= 64 ? ~0ull : (1ull << (n - i0)) - 1);
    const u64 E = H | ~V;                                            // where a group cannot continue: a head, or the end of the input
    const bool valid = (V >> lane) & 1;
    Part x = part_identity<MODE>();
    if (valid) { x.mx = __builtin_nontemporal_load(tri + 3 * i + 2); if (MODE != LINK_NONE) x.v = __builtin_nontemporal_load(vals + i); }
    const u64 below = E & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
    const int hp = below ? 63 - __builtin_clzll(below) : -1, lo = hp < 0 ? 0 : hp;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
      const int om = __shfl_up(x.mx, dd);
      const i64 ov = MODE != LINK_NONE ? __shfl_up(x.v, dd) : 0;
      if (lane - dd >= lo) { x.mx = max(x.mx, om); x.v = val_comb<MODE>(ov, x.v); }
    }
    x.cnt = (unsigned)(lane - lo + 1);
    Part last; last.cnt = __shfl(x.cnt, 63); last.mx = __shfl(x.mx, 63); last.v = MODE != LINK_NONE ? __shfl(x.v, 63) : 0;
    const i64 g = rowBase + __popcll(H & below) - 1;                  // the group of this lane's region
    if (valid && ((H >> lane) & 1) && g < nGroups) headOut[g] = (unsigned)i;
    if (E) {
      const int p0 = __builtin_ctzll(E);
      if (lane == (p0 ? p0 - 1 : 0)) {                               // the group that reaches into this row ends here
        const Part tot = p0 ? part_comb<MODE>(carry, x) : carry;
        if (leftOpen) shA[w] = tot;
        else if (tot.cnt) put_whole<MODE>(rowBase - 1, nGroups, tot, cntOut, stopOut, valOut);
      }
      if (valid && lane < 63 && ((E >> (lane + 1)) & 1) && hp >= 0) put_whole<MODE>(g, nGroups, x, cntOut, stopOut, valOut);   // head and end in this row
      leftOpen = false;
      if (V >> 63) carry = last; else { carry = part_identity<MODE>(); dead = true; }
    } else carry = part_comb<MODE>(carry, last);
  }
  const i64 gB = tb + __shfl(incl, w * kLinkRows + kLinkRows - 1) - 1;
  if (lane == 0) {
    if (leftOpen) { shA[w] = carry; shClosed[w] = 0; shHasB[w] = 0; }
    else { shClosed[w] = 1; shHasB[w] = !dead; shB[w] = carry; }
    shGB[w] = gB;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  Part acc = part_identity<MODE>();
  bool openLeft = true;
  i64 g = tb - 1;
  for (int j = 0; j < kWaves; j++) {
    acc = part_comb<MODE>(acc, shA[j]);
    if (!shClosed[j]) continue;
    if (acc.cnt) { if (openLeft) put_piece<MODE>(g, nGroups, acc, cntOut, stopOut, valOut); else put_whole<MODE>(g, nGroups, acc, cntOut, stopOut, valOut); }
    openLeft = false;
    acc = shHasB[j] ? shB[j] : part_identity<MODE>();
    g = shGB[j];
  }
  if (acc.cnt) {
    const bool nextHead = tileBase + kLinkTile >= n || (bits[(t + 1) * (kLinkTile / 64)] & 1);
    if (nextHead && !openLeft) put_whole<MODE>(g, nGroups, acc, cntOut, stopOut, valOut); else put_piece<MODE>(g, nGroups, acc, cntOut, stopOut, valOut);
  }
}

__global__ __launch_bounds__(256) void link_append_kernel(const int *__restrict__ src, i64 n, int nChrom, int byStrand, int *__restrict__ dst,
                                                         unsigned char *__restrict__ minus, int *bad)
{
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    const int c = src[3 * i];
    if (c < 0 || c >= 2 * nChrom) { atomicOr(bad, 32); continue; }
    const int m = c >= nChrom, id = m ? c - nChrom : c;
    dst[3 * i] = byStrand ? 2 * id + m : id; dst[3 * i + 1] = src[3 * i + 1]; dst[3 * i + 2] = src[3 * i + 2];
    minus[i] = (unsigned char)m;
  }
}

__global__ __launch_bounds__(256) void link_head_keys_kernel(const int *__restrict__ tri, const unsigned char *__restrict__ minus, const unsigned *__restrict__ head,
                                                            const LinkInfo *info, int byStrand, int2 *__restrict__ out)
{
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= info->nGroups) return;
  const i64 h = head[g];
  const int c = tri[3 * h];
  out[g] = make_int2(2 * (byStrand ? c >> 1 : c) + minus[h], tri[3 * h + 1]);
}

template <int MODE>
void launch_groups(const int *tri, const i64 *vals, i64 n, i64 nt, const LinkWork &w, unsigned *headOut, unsigned *countOut, int *stopOut, i64 *valOut, hipStream_t st)
{
  hipLaunchKernelGGL(link_init_kernel<MODE>, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, (const u64 *)w.bits, (const i64 *)w.tileHeadBase, nt,
                     (const LinkInfo *)w.info, countOut, stopOut, valOut);
  hipLaunchKernelGGL(link_groups_kernel<MODE>, dim3((unsigned)nt), dim3(kLinkThreads), 0, st, tri, vals, n, (const u64 *)w.bits, (const i64 *)w.tileHeadBase,
                     (const LinkInfo *)w.info, headOut, countOut, stopOut, valOut);
}

}  // namespace

hipError_t launch_link_append(const int *src, long long n, int nChrom, int byStrand, int *dst, unsigned char *minus, int *bad, hipStream_t st)
{
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
  hipLaunchKernelGGL(link_append_kernel, dim3(grid), dim3(256), 0, st, src, n, nChrom, byStrand, dst, minus, bad);
  return hipGetLastError();
}

hipError_t launch_link_head_keys(const int *tri, const unsigned char *minus, const unsigned *head, const LinkInfo *info, long long n, int byStrand, int2 *out,
                                 hipStream_t st)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(link_head_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tri, minus, head, info, byStrand, out);
  return hipGetLastError();
}

hipError_t launch_link(const int *tri, const long long *vals, long long n, long long maxDifference, int mode, const LinkWork &w,
                       unsigned *headOut, unsigned *countOut, int *stopOut, long long *valOut, hipStream_t st)
{
  const i64 nt = link_tiles(n);
  hipError_t e = hipMemsetAsync(w.info, 0xff, sizeof(u64), st);       // firstUnsorted = none
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(link_scan_kernel<false>, dim3((unsigned)nt), dim3(kLinkThreads), 0, st, tri, n, maxDifference, (const int2 *)nullptr, w.tileAgg,
                     &w.info->firstUnsorted, (u64 *)nullptr, (unsigned *)nullptr);
  hipLaunchKernelGGL(link_prefix_kernel, dim3(1), dim3(kPartThreads), 0, st, (const int2 *)w.tileAgg, nt, w.tilePrefix);
  hipLaunchKernelGGL(link_scan_kernel<true>, dim3((unsigned)nt), dim3(kLinkThreads), 0, st, tri, n, maxDifference, (const int2 *)w.tilePrefix, (int2 *)nullptr,
                     (u64 *)nullptr, w.bits, w.tileHeads);
  hipLaunchKernelGGL(link_heads_kernel, dim3(1), dim3(kPartThreads), 0, st, (const unsigned *)w.tileHeads, nt, w.tileHeadBase, (const u64 *)w.bits, w.info);
  switch (mode) {
    case LINK_SUM: launch_groups<LINK_SUM>(tri, vals, n, nt, w, headOut, countOut, stopOut, valOut, st); break;
    case LINK_MIN: launch_groups<LINK_MIN>(tri, vals, n, nt, w, headOut, countOut, stopOut, valOut, st); break;
    case LINK_MAX: launch_groups<LINK_MAX>(tri, vals, n, nt, w, headOut, countOut, stopOut, valOut, st); break;
    default: launch_groups<LINK_NONE>(tri, vals, n, nt, w, headOut, countOut, stopOut, valOut, st); break;
  }
  return hipGetLastError();
}

}  // namespace gtx
