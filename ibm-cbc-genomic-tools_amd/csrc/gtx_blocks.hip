// Kernels of the block operations (see gtx_blocks.h, which has the shape of the passes).
#include "gtx_blocks.h"
#include "gtx_compact.h"
#include "gtx_textline.h"
#include "gtx_lineout.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;

using gtxtext::digits;
using gtxtext::signed_len;
using gtxtext::put_signed;
using gtxline::line_begin;
using gtxline::tile_exclusive;
using gtxline::store_run;

// ---- the plain line's grammar (include/gtx.h) -------------------------------------------------------------------------------------
struct Tok { unsigned a, z; bool last; };

// the token at p: [a, z), none of its bytes at or below ' '; p moves behind the tab that ends it.  false: empty, or such a byte
__device__ __forceinline__ bool next_tok(const unsigned char *__restrict__ s, unsigned &p, unsigned e, Tok &t)
{
  t.a = p;
  while (p < e && s[p] != '\t') { if (s[p] <= ' ') return false; p++; }
  t.z = p; t.last = p >= e; p++;
  return t.z > t.a;
}

// a canonical decimal of at most 10 digits: "0", or no leading zero
__device__ __forceinline__ bool canon(const unsigned char *__restrict__ s, unsigned a, unsigned z, u64 &v)
{
  const unsigned n = z - a;
  v = 0;
  if (n == 0 || n > 10 || (n > 1 && s[a] == '0')) return false;
  for (unsigned k = a; k < z; k++) { const unsigned c = (unsigned)(s[k] - '0'); if (c >= 10u) return false; v = v * 10 + c; }
  return true;
}

// the list's element at p, which a comma or the list's end z ends; p moves to that byte
__device__ __forceinline__ bool list_item(const unsigned char *__restrict__ s, unsigned &p, unsigned z, u64 &v)
{
  const unsigned a = p;
  while (p < z && s[p] != ',') p++;
  return canon(s, a, p, v);
}

// the same of a list that has been checked: p moves behind the comma
__device__ __forceinline__ unsigned read_item(const unsigned char *__restrict__ s, unsigned &p, unsigned z)
{
  unsigned v = 0;
  while (p < z && s[p] != ',') { v = v * 10 + (unsigned)(s[p] - '0'); p++; }
  p++;
  return v;
}

// Is the line [b, e) of s plain?  r is filled on the way (all but outLen / outCount).  The lists are walked once, in step.
__device__ __forceinline__ bool parse_line(const unsigned char *__restrict__ s, unsigned b, unsigned e, int kind, BlocksRec &r)
{
  unsigned p = b;
  Tok t;
  u64 v;
  r.nTok = 0; r.lineLen = e - b; r.labelOff = 0; r.labelLen = 0; r.scoreOff = 0; r.scoreLen = 0; r.strandOff = 0; r.rgbOff = 0; r.rgbLen = 0;
  r.sizesOff = 0; r.sizesEnd = 0; r.startsOff = 0; r.startsEnd = 0; r.n = 1; r.sz0 = 0; r.stL = 0; r.sum = 0; r.gaps = 0; r.gA = 0; r.gZ = 0; r.listDigits = 0;
  r.t0 = 0; r.t1 = 0; r.strand = '+'; r.outLen = 0; r.outCount = 0;
  if (!next_tok(s, p, e, t) || t.last) return false;
  r.nameLen = t.z - t.a;
  if (!next_tok(s, p, e, t) || t.last || !canon(s, t.a, t.z, v) || (i64)v + 1 >= kBlocksLimit) return false;
  r.s0 = (int)v;
  if (!next_tok(s, p, e, t) || !canon(s, t.a, t.z, v) || (i64)v >= kBlocksLimit) return false;
  r.e = (int)v;
  r.nTok = 3;
  if (t.last) return true;
  if (!next_tok(s, p, e, t)) return false;
  r.labelOff = t.a - b; r.labelLen = t.z - t.a; r.nTok = 4;
  if (t.last) return true;
  if (!next_tok(s, p, e, t)) return false;
  {                                                               // a canonical long of at most 18 digits
    const bool neg = s[t.a] == '-';
    const unsigned q = t.a + (neg ? 1 : 0), nd = t.z - q;
    if (nd == 0 || nd > 18) return false;
    for (unsigned k = q; k < t.z; k++) if ((unsigned)(s[k] - '0') >= 10u) return false;
    if (s[q] == '0' && (nd > 1 || neg)) return false;
  }
  r.scoreOff = t.a - b; r.scoreLen = t.z - t.a; r.nTok = 5;
  if (t.last) return true;
  if (!next_tok(s, p, e, t) || t.z - t.a != 1 || (s[t.a] != '+' && s[t.a] != '-')) return false;
  r.strandOff = t.a - b; r.strand = s[t.a]; r.nTok = 6;
  if (t.last) return true;
  // 7 to 11 columns are not plain: from here on the line has exactly 12
  if (!next_tok(s, p, e, t) || t.last || !canon(s, t.a, t.z, v) || (i64)v >= kBlocksLimit) return false;
  r.t0 = (int)v;
  if (!next_tok(s, p, e, t) || t.last || !canon(s, t.a, t.z, v) || (i64)v >= kBlocksLimit) return false;
  r.t1 = (int)v;
  if (!next_tok(s, p, e, t) || t.last) return false;
  r.rgbOff = t.a - b; r.rgbLen = t.z - t.a;
  if (!next_tok(s, p, e, t) || t.last || !canon(s, t.a, t.z, v) || v < 1 || v > (u64)kBlocksMax) return false;
  r.n = (unsigned)v;
  Tok ts, tt;
  if (!next_tok(s, p, e, ts) || ts.last) return false;
  if (!next_tok(s, p, e, tt) || !tt.last) return false;
  r.nTok = 12;
  unsigned ps = ts.a, pt = tt.a;
  u64 prevEnd = 0, sum = 0, listDigits = 0;
  const u64 s0 = (u64)r.s0;
  for (unsigned k = 0; k < r.n; k++) {
    u64 sz, st;
    if (!list_item(s, ps, ts.z, sz) || !list_item(s, pt, tt.z, st)) return false;
    if (sz < 1 || (k == 0 ? st != 0 : st < prevEnd)) return false;   // the first block begins at column 2; a block begins behind the stop of the one before
    if (s0 + st + sz >= (u64)kBlocksLimit) return false;
    if (k == 0) r.sz0 = (unsigned)sz;
    if (kind == kBlocksSplit) listDigits += (u64)(digits(s0 + st) + digits(s0 + st + sz));
    else if (kind == kBlocksDiff && k > 0 && st > prevEnd) {
      if (r.gaps == 0) r.gA = (unsigned)prevEnd;
      r.gaps++; r.gZ = (unsigned)st;
      listDigits += (u64)(digits(st - prevEnd) + digits(prevEnd - r.gA));
    }
    r.stL = (unsigned)st;
    sum += sz; prevEnd = st + sz;
    if (k + 1 < r.n) {                                            // one comma between two elements
      if (ps >= ts.z || pt >= tt.z) return false;
      ps++; pt++;
    }
  }
  r.sizesOff = ts.a - b; r.sizesEnd = ps - b; r.startsOff = tt.a - b; r.startsEnd = pt - b;
  if (ps < ts.z && s[ps] == ',') ps++;                            // one trailing comma, or none
  if (pt < tt.z && s[pt] == ',') pt++;
  if (ps != ts.z || pt != tt.z) return false;
  if (s0 + prevEnd != (u64)r.e) return false;                     // the last block ends at column 3
  r.sum = (unsigned)sum; r.listDigits = (unsigned)listDigits;
  return true;
}

// ---- the printed line, counted or written ---------------------------------------------------------------------------------------
struct CountSink {
  u64 n = 0;
  __device__ __forceinline__ void ch(unsigned char) { n++; }
  __device__ __forceinline__ void copy(const unsigned char *, unsigned len) { n += len; }
  __device__ __forceinline__ void num(i64 v) { n += (u64)signed_len(v); }
};
struct ByteSink {
  unsigned char *p;
  __device__ __forceinline__ void ch(unsigned char c) { *p++ = c; }
  __device__ __forceinline__ void copy(const unsigned char *__restrict__ src, unsigned len) { for (unsigned k = 0; k < len; k++) p[k] = src[k]; p += len; }
  __device__ __forceinline__ void num(i64 v) { p = put_signed(p, v); }
};

__device__ __forceinline__ bool selects_first(const BlocksOp &op, int strand)
{ return (op.select & kBlocksFirst) || ((op.select & kBlocks5p) && strand == '+') || ((op.select & kBlocks3p) && strand == '-'); }
__device__ __forceinline__ bool selects_last(const BlocksOp &op, int strand)
{ return (op.select & kBlocksLast) || ((op.select & kBlocks5p) && strand == '-') || ((op.select & kBlocks3p) && strand == '+'); }

// one line of split (PrintModified): CHROM TAB A TAB Z TAB LABEL TAB SCORE TAB STRAND NL
template <class Sink>
__device__ __forceinline__ void split_line(Sink &o, const unsigned char *__restrict__ L, const BlocksRec &r, i64 A, i64 Z)
{
  o.copy(L, r.nameLen); o.ch('\t'); o.num(A); o.ch('\t'); o.num(Z); o.ch('\t');
  if (r.labelLen) o.copy(L + r.labelOff, r.labelLen); else o.ch('_');
  o.ch('\t');
  if (r.scoreLen) o.copy(L + r.scoreOff, r.scoreLen); else o.ch('0');
  o.ch('\t'); o.ch((unsigned char)r.strand); o.ch('\n');
}
// the bytes of such a line beside its two numbers
__device__ __forceinline__ unsigned split_fixed(const BlocksRec &r) { return r.nameLen + (r.labelLen ? r.labelLen : 1) + (r.scoreLen ? r.scoreLen : 1) + 7; }

// The line that connect, select, diff, n or strand prints for the line at L, or nothing.  COUNT: the fresh lists of diff are taken
// from the plan's digit count instead of being walked.
template <class Sink, bool COUNT>
__device__ __forceinline__ void render_one(Sink &o, const BlocksOp &op, const unsigned char *__restrict__ L, const BlocksRec &r)
{
  // Print's columns 1 to 6 and 7 to 9 of a 12-column region that spans (A, Z]: UpdateThick on the way
  auto head = [&](i64 A, i64 Z) {
    o.copy(L, r.nameLen); o.ch('\t'); o.num(A); o.ch('\t'); o.num(Z); o.ch('\t');
    o.copy(L + r.labelOff, r.labelLen); o.ch('\t'); o.copy(L + r.scoreOff, r.scoreLen); o.ch('\t'); o.ch((unsigned char)r.strand);
    i64 t0 = max((i64)r.t0, A), t1 = min((i64)r.t1, Z);
    if (t1 <= t0) t0 = t1 = A;
    o.ch('\t'); o.num(t0); o.ch('\t'); o.num(t1); o.ch('\t'); o.copy(L + r.rgbOff, r.rgbLen); o.ch('\t');
  };
  const i64 s0 = r.s0, e = r.e;
  switch (op.kind) {
    case kBlocksStrand: {
      const int ns = op.strandOp == kBlocksPlus ? '+' : op.strandOp == kBlocksMinus ? '-' : (r.strand == '+' ? '-' : '+');
      if (r.nTok < 6) o.copy(L, r.lineLen);
      else {
        o.copy(L, r.strandOff); o.ch((unsigned char)ns);
        if (r.nTok == 12) {
          o.copy(L + r.strandOff + 1, r.sizesEnd - (r.strandOff + 1)); o.ch('\t');
          o.copy(L + r.startsOff, r.startsEnd - r.startsOff);
        }
      }
      o.ch('\n');
      break;
    }
    case kBlocksConnect:
      if (r.nTok < 12) o.copy(L, r.lineLen);
      else { head(s0, e); o.ch('1'); o.ch('\t'); o.num(e - s0); o.ch('\t'); o.ch('0'); }
      o.ch('\n');
      break;
    case kBlocksSelect: {
      const bool pf = selects_first(op, r.strand), pl = selects_last(op, r.strand);
      if (!pf && !pl) break;
      if (r.nTok < 12) { o.copy(L, r.lineLen); o.ch('\n'); break; }
      const i64 z0 = s0 + r.sz0, a1 = s0 + r.stL;                 // the first block is (s0, z0], the last (a1, e]
      if (r.n == 1) { head(s0, e); o.ch('1'); o.ch('\t'); o.num(e - s0); o.ch('\t'); o.ch('0'); }
      else if (pf && pl) { head(s0, e); o.ch('2'); o.ch('\t'); o.num(z0 - s0); o.ch(','); o.num(e - a1); o.ch('\t'); o.ch('0'); o.ch(','); o.num(a1 - s0); }
      else if (pf) { head(s0, z0); o.ch('1'); o.ch('\t'); o.num(z0 - s0); o.ch('\t'); o.ch('0'); }
      else { head(a1, e); o.ch('1'); o.ch('\t'); o.num(e - a1); o.ch('\t'); o.ch('0'); }
      o.ch('\n');
      break;
    }
    case kBlocksDiff: {
      if (r.nTok < 12 || r.gaps == 0) break;
      head(s0 + r.gA, s0 + r.gZ);
      o.num(r.gaps); o.ch('\t');
      if constexpr (COUNT) o.n += (u64)r.listDigits + 2 * (r.gaps - 1) + 1;   // the digits, the commas of both lists, the tab between them
      else {
        for (int pass = 0; pass < 2; pass++) {                    // the gaps' sizes, then their starts from the first one's
          unsigned ps = r.sizesOff, pt = r.startsOff, prevEnd = 0, seen = 0;
          for (unsigned k = 0; k < r.n; k++) {
            const unsigned sz = read_item(L, ps, r.sizesEnd), st = read_item(L, pt, r.startsEnd);
            if (k > 0 && st > prevEnd) {
              if (seen++) o.ch(',');
              o.num(pass == 0 ? (i64)(st - prevEnd) : (i64)(prevEnd - r.gA));
            }
            prevEnd = st + sz;
          }
          if (pass == 0) o.ch('\t');
        }
      }
      o.ch('\n');
      break;
    }
    default:                                                      // n: LABEL TAB the sum of the sizes, 0 for an interval with start > stop
      if (r.labelLen) o.copy(L + r.labelOff, r.labelLen); else o.ch('_');
      o.ch('\t');
      o.num(r.nTok == 12 ? (i64)r.sum : (s0 + 1 > e ? 0 : e - s0));
      o.ch('\n');
  }
}

// ---- plan ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlocksTile) void blocks_plan_kernel(BlocksDevice d, BlocksOp op)
{
  const unsigned tile = blockIdx.x, j = tile * kBlocksTile + threadIdx.x;
  // the index: as many newlines as the caller counted, the last of them the block's last byte
  if (*d.nlTotal != d.nLines) {
    if (threadIdx.x == 0) { atomicOr(d.flag, 1); d.tileBytes[tile] = 0; d.tileCount[tile] = 0; }
    return;
  }
  unsigned len = 0, count = 0;
  if (j < d.nLines) {
    const unsigned b = line_begin(d.nl, j), e = d.nl[j];
    const unsigned char *s = (const unsigned char *)d.text;
    BlocksRec r = {};
    bool ok = b <= e && (size_t)e < d.bytes && (j + 1 < d.nLines || (size_t)e + 1 == d.bytes) && parse_line(s, b, e, op.kind, r);
    if (ok) {
      u64 bytes;
      if (op.kind == kBlocksSplit) {
        count = r.n;
        bytes = r.nTok == 12 ? (u64)r.n * split_fixed(r) + r.listDigits : (u64)split_fixed(r) + (u64)(signed_len(r.s0) + signed_len(r.e));
      } else {
        CountSink o;
        render_one<CountSink, true>(o, op, s + b, r);
        bytes = o.n; count = bytes ? 1 : 0;
      }
      if (bytes > kBlocksLineMax) { atomicOr(d.flag, 32); ok = false; count = 0; }
      else len = (unsigned)bytes;
    } else atomicOr(d.flag, 16);
    r.outLen = len; r.outCount = count;
    d.rec[j] = r;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { len += __shfl_xor(len, o); count += __shfl_xor(count, o); }
  if (threadIdx.x == 0) {
    if (op.kind != kBlocksSplit && len > (unsigned)kBlocksStage) atomicOr(d.flag, 32);
    d.tileBytes[tile] = len; d.tileCount[tile] = count;
  }
}

// split: the lines' exclusive sums of printed lines and bytes, [nLines] the totals
__global__ __launch_bounds__(kBlocksTile) void blocks_base_kernel(BlocksDevice d)
{
  if (*d.flag) return;
  const unsigned tile = blockIdx.x, j = tile * kBlocksTile + threadIdx.x;
  unsigned c = 0; u64 n = 0;
  if (j < d.nLines) { c = d.rec[j].outCount; n = d.rec[j].outLen; }
  const unsigned atC = (unsigned)d.baseCount[tile] + tile_exclusive<kBlocksTile, unsigned>(c, nullptr);   // (one wave: no LDS)
  const i64 atN = d.baseBytes[tile] + (i64)tile_exclusive<kBlocksTile, u64>(n, nullptr);
  if (j < d.nLines) { d.lineOut[j] = atC; d.lineByte[j] = atN; }
  if (j + 1 == d.nLines) { d.lineOut[d.nLines] = atC + c; d.lineByte[d.nLines] = atN + (i64)n; }
}

// ---- emit (the runs go out through store_run, gtx_lineout.h) ------------------------------------------------------------------------
__global__ __launch_bounds__(kBlocksTile) void blocks_emit_kernel(BlocksDevice d, BlocksOp op, char *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) unsigned char run[kBlocksStage + 32];
  if (*d.flag) return;
  const unsigned tile = blockIdx.x, j = tile * kBlocksTile + threadIdx.x;
  const i64 lo = d.baseBytes[tile], hi = d.baseBytes[tile + 1];
  if (hi == lo) return;
  BlocksRec r; r.outLen = 0;
  if (j < d.nLines) r = d.rec[j];
  const unsigned at = tile_exclusive<kBlocksTile, unsigned>(r.outLen, nullptr), pad = (unsigned)(lo & 15);   // pad + (hi - lo) <= 15 + kBlocksStage
  if (r.outLen) {
    ByteSink o; o.p = run + pad + at;
    render_one<ByteSink, false>(o, op, (const unsigned char *)d.text + line_begin(d.nl, j), r);
  }
  __syncthreads();
  store_run<kBlocksTile>(out, run, lo, (unsigned)(hi - lo));
}

__global__ __launch_bounds__(kBlocksOutTile) void blocks_split_kernel(BlocksDevice d, i64 totalLines, char *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) unsigned char run[kBlocksOutStage + 32];
  __shared__ i64 sLo, sHi;
  if (*d.flag) return;
  const i64 o0 = (i64)blockIdx.x * kBlocksOutTile, o = o0 + threadIdx.x;
  const bool mine = o < totalLines;
  BlocksRec r;
  const unsigned char *L = nullptr;
  i64 at = 0, A = 0, Z = 0;
  unsigned len = 0;
  if (mine) {
    unsigned a = 0, z = d.nLines;                                 // the last line j with lineOut[j] <= o
    while (z - a > 1) { const unsigned m = a + (z - a) / 2; if ((i64)d.lineOut[m] <= o) a = m; else z = m; }
    const unsigned j = a, k = (unsigned)(o - d.lineOut[j]);
    r = d.rec[j];
    L = (const unsigned char *)d.text + line_begin(d.nl, j);
    at = d.lineByte[j];
    A = r.s0; Z = r.e;
    if (r.nTok == 12) {                                           // to block k, past the bytes of the blocks in front
      const unsigned fixed = split_fixed(r);
      unsigned ps = r.sizesOff, pt = r.startsOff, sz = 0, st = 0;
      for (unsigned q = 0; q <= k; q++) {
        if (q) at += fixed + (unsigned)(digits((u64)A) + digits((u64)Z));
        sz = read_item(L, ps, r.sizesEnd); st = read_item(L, pt, r.startsEnd);
        A = (i64)r.s0 + st; Z = A + sz;
      }
    }
    len = split_fixed(r) + (unsigned)(signed_len(A) + signed_len(Z));
  }
  if (threadIdx.x == 0) sLo = at;
  if (mine && (o + 1 == totalLines || threadIdx.x == kBlocksOutTile - 1)) sHi = at + len;
  __syncthreads();
  const i64 lo = sLo, total = sHi - sLo;
  if ((lo & 15) + total <= (i64)kBlocksOutStage + 15) {
    if (mine) { ByteSink w; w.p = run + (unsigned)(lo & 15) + (unsigned)(at - lo); split_line(w, L, r, A, Z); }
    __syncthreads();
    store_run<kBlocksOutTile>(out, run, lo, (unsigned)total);
  } else if (mine) {                                              // a run the stage does not hold: every lane stores its own line
    ByteSink w; w.p = (unsigned char *)out + at;
    split_line(w, L, r, A, Z);
  }
}

}  // namespace

hipError_t launch_blocks_plan(const BlocksDevice &d, const BlocksOp &op, hipStream_t st)
{
  if (d.nLines == 0) return hipSuccess;
  const unsigned nTiles = (unsigned)blocks_tiles(d.nLines);
  blocks_plan_kernel<<<nTiles, kBlocksTile, 0, st>>>(d, op);
  hipError_t e = launch_tile_prefix(d.tileBytes, (long long)nTiles, d.baseBytes, st);
  if (e != hipSuccess) return e;
  e = launch_tile_prefix(d.tileCount, (long long)nTiles, d.baseCount, st);
  if (e != hipSuccess) return e;
  if (op.kind == kBlocksSplit) blocks_base_kernel<<<nTiles, kBlocksTile, 0, st>>>(d);
  return hipGetLastError();
}

hipError_t launch_blocks_emit(const BlocksDevice &d, const BlocksOp &op, long long totalLines, char *out, hipStream_t st)
{
  if (d.nLines == 0 || totalLines <= 0) return hipSuccess;
  if (op.kind == kBlocksSplit) {
    const unsigned grid = (unsigned)((totalLines + kBlocksOutTile - 1) / kBlocksOutTile);
    blocks_split_kernel<<<grid, kBlocksOutTile, 0, st>>>(d, totalLines, out);
  } else blocks_emit_kernel<<<(unsigned)blocks_tiles(d.nLines), kBlocksTile, 0, st>>>(d, op, out);
  return hipGetLastError();
}

}  // namespace gtx
