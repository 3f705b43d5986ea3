// Kernels of the sliding windows (see gtx_windows.h, which has the shape of the passes).
#include "gtx_windows.h"
#include "gtx_compact.h"
#include "gtx_textline.h"
#include "gtx_lineout.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef long long i64x2 __attribute__((ext_vector_type(2)));
using gtxtext::digits;
using gtxtext::put_signed;
using gtxline::line_begin;
using gtxline::stage_text;
using gtxline::tile_total;
using gtxline::tile_exclusive;
using gtxline::store_run;

constexpr int kStageBytes = kWindowsStage + 32;   // a stage begins at the 16-byte line below its first byte and is filled in whole units
constexpr int kRunBytes = kWindowsRunBytes + 32;  // ... and so does a run

// digits(a) + digits(a + d) + .. over m terms; 0 <= a, 1 <= d <= 2^31, every term below 10^10.  Term i has more than j digits from
// i = k_j on, k_j = 0 when a >= 10^j, else ceil((10^j - a) / d): the k_j do not decrease with j
__device__ __forceinline__ i64 progression_digits(i64 a, i64 d, i64 m)
{
  i64 sum = m, p = 10;
#pragma unroll 1
  for (int j = 1; j <= 9; j++, p *= 10) {
    const i64 kj = a >= p ? 0 : (i64)(((unsigned)(p - a) + (unsigned)(d - 1)) / (unsigned)d);   // (10^9 + 2^31 - 1 < 2^32)
    if (kj >= m) break;
    sum += m - kj;
  }
  return sum;
}

__device__ __forceinline__ unsigned fixed_len(const WindowsRec &r) { return (unsigned)r.nameLen + 2u + r.tailLen + 1u; }

// the bytes of the first k windows of a line, k <= n
__device__ __forceinline__ i64 bytes_before(const WindowsRec &r, const WindowsOp &op, i64 k)
{
  if (k == 0) return 0;
  const i64 full = min(k, r.c);
  return k * (i64)fixed_len(r) + progression_digits(r.v2, op.step, k) + progression_digits((i64)r.v2 + op.size, op.step, full) + (k - full) * digits((u64)r.stop);
}

// the largest j in [lo, hi) with P[j] <= o; P[lo] <= o holds
template <class PTR>
__device__ __forceinline__ unsigned find_line(PTR P, unsigned lo, unsigned hi, i64 o)
{
  while (hi - lo > 1) {
    const unsigned mid = lo + (hi - lo) / 2;
    if (P[mid] <= o) lo = mid; else hi = mid;
  }
  return lo;
}

// n bytes of the block's text into a run, eight loads in flight at a time: one at a time a window waits for the latency of every
// byte of its name and tail in turn
__device__ __forceinline__ void copy_bytes(unsigned char *p, const char *__restrict__ src, unsigned n)
{
  for (unsigned q0 = 0; q0 < n; q0 += 8) {
    unsigned char t[8];
#pragma unroll
    for (unsigned u = 0; u < 8; u++) t[u] = q0 + u < n ? (unsigned char)src[q0 + u] : (unsigned char)0;
#pragma unroll
    for (unsigned u = 0; u < 8; u++) if (q0 + u < n) p[q0 + u] = t[u];
  }
}

// the same with the 64 lanes of a wave probing 64 places a step (o, lo and hi the same in all of them, all of them active): a search
// over ten million lines is four dependent loads instead of twenty-three
__device__ __forceinline__ unsigned find_line_wave(const i64 *__restrict__ P, unsigned lo, unsigned hi, i64 o)
{
  const unsigned lane = threadIdx.x & 63;
  while (hi - lo > 1) {
    const unsigned step = (hi - lo + 63) / 64, at = lo + lane * step;
    const u64 le = __ballot(at < hi && P[at] <= o);               // a prefix of the lanes: P does not decrease, and lane 0 holds
    const unsigned last = 63u - (unsigned)__clzll(le);
    lo += last * step; hi = min(lo + step, hi);
  }
  return lo;
}

__global__ __launch_bounds__(kWindowsLineTile) void windows_plan_kernel(WindowsDevice d, WindowsOp op)
{
  __shared__ __attribute__((aligned(16))) unsigned char in[kStageBytes];
  __shared__ u64 sBytes, sWindows;
  const unsigned tile = blockIdx.x, j0 = tile * kWindowsLineTile, j1 = min(j0 + kWindowsLineTile, d.nLines);
  // the tokenizer's verdict: nl[] may hold nothing to go by
  if (*d.flag & 7) { if (threadIdx.x == 0) { d.tileBytes[tile] = 0; d.tileWindows[tile] = 0; } return; }
  const size_t t0 = line_begin(d.nl, j0), t1 = (size_t)d.nl[j1 - 1] + 1;
  if (t1 - t0 > (size_t)kWindowsStage) {                          // (the same in every thread of the block)
    if (threadIdx.x == 0) { atomicOr(d.flag, 32); d.tileBytes[tile] = 0; d.tileWindows[tile] = 0; }
    return;
  }
  if (threadIdx.x == 0) { sBytes = 0; sWindows = 0; }
  const size_t a0 = t0 & ~(size_t)15;
  stage_text<kWindowsLineTile>(in, d.text, d.bytes, a0, t1);
  __syncthreads();
  const unsigned j = j0 + threadIdx.x;
  i64 nWin = 0, nBytes = 0;
  if (j < j1) {
    const unsigned b = (unsigned)(line_begin(d.nl, j) - a0), e = (unsigned)((size_t)d.nl[j] - a0);
    gtxtext::LineCols c;
    WindowsRec r; r.n = 0; r.c = 0; r.bytes = 0; r.v2 = 0; r.stop = 0; r.nameOff = 0; r.tailOff = 0; r.nameLen = 0; r.tailLen = 0;
    if (!gtxtext::verbatim_line((const unsigned char *)in, b, e, c) || c.v2 >= 2147483645ll || c.v3 >= 2147483646ll) atomicOr(d.flag, 16);
    else {
      // the tail: nothing, column 4 alone (a 5-column line loses its score), or columns 4 to 6 as they stand
      const unsigned tailLen = c.nTok == 3 ? 0u : c.nTok < 6 ? c.col4End - c.tailOff : (e - b) - c.tailOff;
      if (c.nameLen + 2u + tailLen + 1u > (unsigned)kWindowsMaxFixed) atomicOr(d.flag, 32);
      else {
        const i64 len = c.v3 - c.v2;
        r.c = op.size > len ? 0 : (len - op.size) / op.step + 1;
        r.n = !op.small ? r.c : len <= 0 ? 0 : (len - 1) / op.step + 1;
        r.v2 = (int)c.v2; r.stop = (int)c.v3;
        r.nameOff = (unsigned)(a0 + b); r.tailOff = (unsigned)(a0 + b + c.tailOff); r.nameLen = (unsigned short)c.nameLen; r.tailLen = (unsigned short)tailLen;
        r.bytes = bytes_before(r, op, r.n);
      }
    }
    d.rec[j] = r;
    nWin = r.n; nBytes = r.bytes;
  }
  // the tile's totals: per wave in registers, then one add per wave
  tile_total((u64)nBytes, &sBytes);
  tile_total((u64)nWin, &sWindows);
  __syncthreads();
  if (threadIdx.x == 0) { d.tileBytes[tile] = sBytes; d.tileWindows[tile] = sWindows; }
}

// lineWin / lineByte of a tile's lines: the tile's bases plus the exclusive scan over its lines
__global__ __launch_bounds__(kWindowsLineTile) void windows_base_kernel(WindowsDevice d)
{
  __shared__ i64x2 waveSum[kWindowsLineTile / 64];                // (windows, bytes) of a wave
  if (*d.flag) return;
  const unsigned tile = blockIdx.x, j = tile * kWindowsLineTile + threadIdx.x;
  i64 n = 0, by = 0;
  if (j < d.nLines) { n = d.rec[j].n; by = d.rec[j].bytes; }
  const i64x2 at = tile_exclusive<kWindowsLineTile>(i64x2{n, by}, waveSum);   // both sums in one scan, behind one barrier
  const i64 atN = d.baseWindows[tile] + at.x, atB = d.baseBytes[tile] + at.y;
  if (j < d.nLines) { d.lineWin[j] = atN; d.lineByte[j] = atB; }
  if (j + 1 == d.nLines) { d.lineWin[d.nLines] = atN + n; d.lineByte[d.nLines] = atB + by; }
}

__global__ __launch_bounds__(kWindowsThreads) void windows_emit_kernel(WindowsDevice d, WindowsOp op, WindowsRange rg)
{
  __shared__ __attribute__((aligned(16))) unsigned char run[kRunBytes];
  __shared__ i64 span[kWindowsSpan + 1];
  __shared__ i64 sLo, sHi;
  // (no look at the flag and no load of the total: the host has the plan's verdict and totals before it launches a range, and a
  // block's first bytes wait for every dependent load in front of them)
  const i64 o0 = rg.first + (i64)blockIdx.x * kWindowsOutTile;
  if (o0 >= rg.total) return;                                     // (the host launches no such block)
  const i64 o1 = min(o0 + kWindowsOutTile, rg.total);
  // the line of the tile's first window (the same in every thread); the bases of the kWindowsSpan lines from there on into LDS, which
  // as a rule hold the line of the tile's last window too
  const unsigned jLo = find_line_wave(d.lineWin, 0u, d.nLines, o0), jEnd = min(jLo + (unsigned)kWindowsSpan, d.nLines);
  for (unsigned k = threadIdx.x; k < jEnd - jLo; k += kWindowsThreads) span[k] = d.lineWin[jLo + k];
  __syncthreads();
  const bool staged = jEnd == d.nLines || span[jEnd - jLo - 1] > o1 - 1;
  const unsigned jHi = staged ? jLo + find_line(span, 0u, jEnd - jLo, o1 - 1) : find_line_wave(d.lineWin, jEnd - 1, d.nLines, o1 - 1);
  // a lane's windows: their lines, their places in the output, their numbers
  unsigned line[kWindowsPerLane], len[kWindowsPerLane];
  i64 off[kWindowsPerLane], k[kWindowsPerLane];
  WindowsRec r;
  unsigned have = ~0u;                                            // the line r holds
  i64 behind = -1;                                                // the byte behind the lane's window in front
#pragma unroll
  for (int i = 0; i < kWindowsPerLane; i++) {
    const i64 o = o0 + (i64)threadIdx.x * kWindowsPerLane + i;
    len[i] = 0; line[i] = 0; off[i] = 0; k[i] = 0;
    if (o >= o1) continue;
    const unsigned j = staged ? jLo + find_line(span, 0u, jHi - jLo + 1, o) : find_line((const i64 *)d.lineWin, jLo, jHi + 1, o);
    const i64 first = staged ? span[j - jLo] : d.lineWin[j];
    if (j != have) { r = d.rec[j]; have = j; }
    line[i] = j; k[i] = o - first;
    // behind the lane's window in front when that is on the same line; else from the line's base by the closed form
    off[i] = k[i] > 0 && behind >= 0 ? behind : d.lineByte[j] + bytes_before(r, op, k[i]);
    const i64 start = (i64)r.v2 + k[i] * op.step, stop = k[i] < r.c ? start + op.size : (i64)r.stop;
    len[i] = fixed_len(r) + (unsigned)digits((u64)start) + (unsigned)digits((u64)stop);
    behind = off[i] + len[i];
    if (o == o0) sLo = off[i];
    if (o == o1 - 1) sHi = off[i] + len[i];
  }
  __syncthreads();
  const i64 lo = sLo, hi = sHi;
  const i64 at = lo - rg.base;                                    // where the run begins in the range's buffer
  const unsigned pad = (unsigned)(at & 15);                       // run[q] is byte at - pad + q of the buffer; pad + (hi - lo) <= 15 + kWindowsRunBytes
#pragma unroll
  for (int i = 0; i < kWindowsPerLane; i++) {
    if (len[i] == 0) continue;
    if (line[i] != have) { r = d.rec[line[i]]; have = line[i]; }
    unsigned char *p = run + pad + (unsigned)(off[i] - lo);
    const char *__restrict__ name = d.text + r.nameOff, *__restrict__ tail = d.text + r.tailOff;
    copy_bytes(p, name, r.nameLen);
    p += r.nameLen;
    const i64 start = (i64)r.v2 + k[i] * op.step;
    *p++ = '\t';
    p = put_signed(p, start);
    *p++ = '\t';
    p = put_signed(p, k[i] < r.c ? start + op.size : (i64)r.stop);
    copy_bytes(p, tail, r.tailLen);
    p[r.tailLen] = '\n';
  }
  __syncthreads();
  store_run<kWindowsThreads>(rg.out, run, at, (unsigned)(hi - lo));
  if (threadIdx.x == 0 && (blockIdx.x + 1 == gridDim.x)) *rg.rangeBytes = (u64)(hi - rg.base);
}

}  // namespace

hipError_t launch_windows_plan(const WindowsDevice &d, const WindowsOp &op, hipStream_t st)
{
  if (d.nLines == 0) return hipSuccess;
  const unsigned nTiles = (unsigned)windows_tiles(d.nLines);
  windows_plan_kernel<<<nTiles, kWindowsLineTile, 0, st>>>(d, op);
  hipError_t e = launch_tile_prefix64(d.tileWindows, (long long)nTiles, d.baseWindows, st);
  if (e != hipSuccess) return e;
  e = launch_tile_prefix64(d.tileBytes, (long long)nTiles, d.baseBytes, st);
  if (e != hipSuccess) return e;
  windows_base_kernel<<<nTiles, kWindowsLineTile, 0, st>>>(d);
  return hipGetLastError();
}

hipError_t launch_windows_emit(const WindowsDevice &d, const WindowsOp &op, const WindowsRange &r, hipStream_t st)
{
  if (r.tiles <= 0) return hipSuccess;
  windows_emit_kernel<<<(unsigned)r.tiles, kWindowsThreads, 0, st>>>(d, op, r);
  return hipGetLastError();
}

}  // namespace gtx
