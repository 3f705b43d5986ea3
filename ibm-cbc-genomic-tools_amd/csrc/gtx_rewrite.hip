// Kernels of the column rewrite (see gtx_rewrite.h, which has the shape of the passes).
#include "gtx_rewrite.h"
#include "gtx_compact.h"
#include "gtx_textline.h"
#include "gtx_lineout.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kStageBytes = kRewriteStage + 32;   // a stage begins at the 16-byte line below its first byte and is filled in whole units

using gtxtext::signed_len;
using gtxtext::put_signed;
using gtxline::line_begin;
using gtxline::stage_text;
using gtxline::tile_total;
using gtxline::tile_exclusive;
using gtxline::store_run;

// the operation on (s, e) of a line on `strand` whose tokenizer class is cls; false: the line is dropped
__device__ __forceinline__ bool apply(const RewriteOp &op, int strand, int cls, i64 &s, i64 &e)
{
  switch (op.kind) {
    case kRewriteShift: s += op.a; e += op.b; return true;
    case kRewriteShiftP:
      if (strand == '-') { s -= op.b; e -= op.a; } else { s += op.a; e += op.b; }
      return true;
    case kRewritePos:
      if (op.posOp == kPosCenter) { const i64 m = s + (e - s + 1) / 2; s = m - op.a; e = m + op.a; }
      else {
        const bool chooseStart = op.posOp == kPosStart || (strand == '+' && op.posOp == kPos5p) || (strand == '-' && op.posOp == kPos3p);
        if (chooseStart) e = s + op.a; else s = e - op.a;
      }
      return true;
    case kRewriteCenter: { const i64 h = (e - s) / 2; s += h; e -= h; return true; }
    case kRewriteFix: return s >= 1 && s <= e;
    default: {                                                    // bounds, then Fix
      if (cls < 0 || cls >= op.nChrom) return false;
      const i64 len = op.chromLen[cls];
      if (s > len || e < 1 || e < s) return false;
      if (s < 1) s = 1;
      if (e > len) e = len;
      return s >= 1 && s <= e;
    }
  }
}

__global__ __launch_bounds__(kRewriteTile) void rewrite_plan_kernel(RewriteDevice d, RewriteOp op)
{
  __shared__ __attribute__((aligned(16))) unsigned char in[kStageBytes];
  __shared__ unsigned sBytes, sLines;
  const unsigned tile = blockIdx.x, j0 = tile * kRewriteTile, j1 = min(j0 + kRewriteTile, d.nLines);
  // the tokenizer's verdict: nl[] may hold nothing to go by
  if (*d.flag & 7) { if (threadIdx.x == 0) { d.tileBytes[tile] = 0; d.tileLines[tile] = 0; } return; }
  const size_t t0 = line_begin(d.nl, j0), t1 = (size_t)d.nl[j1 - 1] + 1;
  if (t1 - t0 > (size_t)kRewriteStage) {                          // (the same in every thread of the block)
    if (threadIdx.x == 0) { atomicOr(d.flag, 32); d.tileBytes[tile] = 0; d.tileLines[tile] = 0; }
    return;
  }
  if (threadIdx.x == 0) { sBytes = 0; sLines = 0; }
  const size_t a0 = t0 & ~(size_t)15;
  stage_text<kRewriteTile>(in, d.text, d.bytes, a0, t1);
  __syncthreads();
  const unsigned j = j0 + threadIdx.x;
  unsigned len = 0;
  if (j < j1) {
    const unsigned b = (unsigned)(line_begin(d.nl, j) - a0), e = (unsigned)((size_t)d.nl[j] - a0);
    gtxtext::LineCols c;
    RewriteRec r; r.s0 = 0; r.e1 = 0; r.nameLen = 0; r.tailOff = 0; r.outLen = 0; r.pad = 0;
    if (!gtxtext::verbatim_line((const unsigned char *)in, b, e, c)) atomicOr(d.flag, 16);
    else {
      i64 s = c.v2 + 1, en = c.v3;
      if (apply(op, c.strand, op.kind == kRewriteBounds ? d.tri[3 * (size_t)j] : -1, s, en)) {
        r.s0 = s - 1; r.e1 = en; r.nameLen = c.nameLen; r.tailOff = c.tailOff;
        r.outLen = c.nameLen + 1 + (unsigned)signed_len(r.s0) + 1 + (unsigned)signed_len(r.e1) + (e + 1 - (b + c.tailOff));
      }
    }
    d.rec[j] = r;
    len = r.outLen;
  }
  // the tile's totals: per wave in registers, then one add per wave
  tile_total(len, &sBytes);
  const u64 kept = __ballot(len != 0);
  if ((threadIdx.x & 63) == 0) atomicAdd(&sLines, (unsigned)__popcll(kept));
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sBytes > (unsigned)kRewriteStage) atomicOr(d.flag, 32);
    d.tileBytes[tile] = sBytes; d.tileLines[tile] = sLines;
  }
}

__global__ __launch_bounds__(kRewriteTile) void rewrite_emit_kernel(RewriteDevice d)
{
  __shared__ __attribute__((aligned(16))) unsigned char in[kStageBytes];
  __shared__ __attribute__((aligned(16))) unsigned char run[kStageBytes];
  __shared__ unsigned waveSum[kRewriteTile / 64];
  if (*d.flag) return;
  const unsigned tile = blockIdx.x, j0 = tile * kRewriteTile, j1 = min(j0 + kRewriteTile, d.nLines);
  const i64 lo = d.baseBytes[tile], hi = d.baseBytes[tile + 1];
  if (hi == lo) return;                                           // nothing kept here
  const size_t t0 = line_begin(d.nl, j0), t1 = (size_t)d.nl[j1 - 1] + 1, a0 = t0 & ~(size_t)15;
  stage_text<kRewriteTile>(in, d.text, d.bytes, a0, t1);
  const unsigned j = j0 + threadIdx.x;
  RewriteRec r; r.outLen = 0;
  if (j < j1) r = d.rec[j];
  const unsigned at = tile_exclusive<kRewriteTile>(r.outLen, waveSum);   // where the line begins inside the run (its barrier: `in` is staged)
  const unsigned pad = (unsigned)(lo & 15);                       // run[k] is byte lo - pad + k of the output; pad + (hi - lo) <= 15 + kRewriteStage
  if (r.outLen) {
    const unsigned b = (unsigned)(line_begin(d.nl, j) - a0), e = (unsigned)((size_t)d.nl[j] - a0);
    unsigned char *p = run + pad + at;
    for (unsigned k = 0; k < r.nameLen; k++) p[k] = in[b + k];
    p += r.nameLen;
    *p++ = '\t';
    p = put_signed(p, r.s0);
    *p++ = '\t';
    p = put_signed(p, r.e1);
    for (unsigned k = b + r.tailOff; k <= e; k++) *p++ = in[k];   // the tail, the newline included
  }
  __syncthreads();
  store_run<kRewriteTile>(d.out, run, lo, (unsigned)(hi - lo));
}

}  // namespace

hipError_t launch_rewrite(const RewriteDevice &d, const RewriteOp &op, hipStream_t st)
{
  if (d.nLines == 0) return hipSuccess;
  const unsigned nTiles = (unsigned)rewrite_tiles(d.nLines);
  rewrite_plan_kernel<<<nTiles, kRewriteTile, 0, st>>>(d, op);
  hipError_t e = launch_tile_prefix(d.tileBytes, (long long)nTiles, d.baseBytes, st);
  if (e != hipSuccess) return e;
  e = launch_tile_prefix(d.tileLines, (long long)nTiles, d.baseLines, st);
  if (e != hipSuccess) return e;
  rewrite_emit_kernel<<<nTiles, kRewriteTile, 0, st>>>(d);
  return hipGetLastError();
}

}  // namespace gtx
