// Kernels of the format conversion (see gtx_convert.h, which has the shape of the passes).
#include "gtx_convert.h"
#include "gtx_compact.h"
#include "gtx_textline.h"
#include "gtx_lineout.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kStageBytes = kConvertStage + 32;   // a run begins inside its first 16-byte unit and is read out in whole units

using gtxtext::signed_len;
using gtxtext::put_signed;
using gtxline::line_begin;
using gtxline::tile_total;
using gtxline::tile_exclusive;
using gtxline::store_run;

// The walks below run on lines launch_tokenize has judged plain (gtx.h has the grammar), so they test nothing again; every loop still
// ends at the line's end e, whatever the bytes are.

// the token at p: p moves to the tab behind it (or to e)
__device__ __forceinline__ void skip_token(const unsigned char *__restrict__ s, unsigned &p, unsigned e) { while (p < e && s[p] != '\t') p++; }

// the decimal at p: p moves to the byte behind its digits
__device__ __forceinline__ u64 read_number(const unsigned char *__restrict__ s, unsigned &p, unsigned e)
{
  u64 v = 0;
  while (p < e && (unsigned)(s[p] - '0') < 10u) { v = v * 10 + (unsigned)(s[p] - '0'); p++; }
  return v;
}

// one SAM alignment [b, e): QNAME, FLAG's strand bit, RNAME, POS and the CIGAR's reference length (M D X; "*" reads as len(SEQ) M)
__device__ __forceinline__ void walk_sam(const unsigned char *__restrict__ s, unsigned b, unsigned e, ConvertRec &r)
{
  unsigned p = b;
  skip_token(s, p, e);
  r.labelOff = 0; r.labelLen = p - b;
  p++;
  const u64 flag = read_number(s, p, e);
  r.strand = (flag & 0x10) ? '-' : '+';
  p++;
  r.chromOff = p - b;
  skip_token(s, p, e);
  r.chromLen = p - b - r.chromOff;
  p++;
  const i64 pos = (i64)read_number(s, p, e);
  p++;
  skip_token(s, p, e);                                            // MAPQ
  p++;
  i64 ref = 0;
  if (p + 1 < e && s[p] == '*' && s[p + 1] == '\t') {
    p += 2;
    skip_token(s, p, e); p++;                                     // RNEXT
    skip_token(s, p, e); p++;                                     // PNEXT
    skip_token(s, p, e); p++;                                     // TLEN
    const unsigned q = p;
    skip_token(s, p, e);
    ref = p - q;
  } else {
    while (p < e && s[p] != '\t') {
      const i64 v = (i64)read_number(s, p, e);
      if (p >= e) break;
      const unsigned char op = s[p++];
      if (op == 'M' || op == 'X' || op == 'D') ref += v;
    }
  }
  r.s0 = (int)(pos - 1); r.e = (int)(pos + ref - 1);
}

// one GFF / GTF feature [b, e): columns 1, 4, 5, 7 and 9 (an 8-column line has the label "_": labelLen 0)
__device__ __forceinline__ void walk_gff(const unsigned char *__restrict__ s, unsigned b, unsigned e, ConvertRec &r)
{
  unsigned p = b;
  skip_token(s, p, e);
  r.chromOff = 0; r.chromLen = p - b;
  p++;
  skip_token(s, p, e); p++;                                       // source
  skip_token(s, p, e); p++;                                       // feature
  const i64 v4 = (i64)read_number(s, p, e);
  p++;
  const i64 v5 = (i64)read_number(s, p, e);
  p++;
  skip_token(s, p, e); p++;                                       // score
  r.strand = p < e ? s[p] : '+';
  p += 2;
  skip_token(s, p, e);                                            // frame
  r.labelOff = 0; r.labelLen = 0;
  if (p < e) {
    const unsigned q = ++p;
    skip_token(s, p, e);
    r.labelOff = q - b; r.labelLen = p - q;
  }
  r.s0 = (int)(v4 - 1); r.e = (int)v5;
}

// the bytes of the printed line
__device__ __forceinline__ unsigned out_len(const ConvertOp &op, const ConvertRec &r)
{
  const unsigned label = r.labelLen ? r.labelLen : 1;
  if (op.to == kConvertReg) return label + 1 + r.chromLen + 3 + (unsigned)signed_len((i64)r.s0 + 1) + 1 + (unsigned)signed_len(r.e) + 1;
  const unsigned nums = (unsigned)signed_len(r.s0) + 1 + (unsigned)signed_len(r.e);
  unsigned n = (op.ucsc ? 3 : 0) + r.chromLen + 1 + nums + 1 + label + 6 + 1 + 1;
  if (op.colorLen) n += 1 + nums + 1 + (unsigned)op.colorLen;
  return n;
}

__global__ __launch_bounds__(kConvertTile) void convert_plan_kernel(ConvertDevice d, ConvertOp op)
{
  __shared__ unsigned sBytes;
  const unsigned tile = blockIdx.x, j0 = tile * kConvertTile, j1 = min(j0 + kConvertTile, d.nLines);
  // the tokenizer's verdict: a block with a line that is not plain is not walked (nl[] may hold nothing to go by)
  if (*d.flag & 7) { if (threadIdx.x == 0) d.tileBytes[tile] = 0; return; }
  if (threadIdx.x == 0) sBytes = 0;
  __syncthreads();
  const unsigned j = j0 + threadIdx.x;
  unsigned len = 0;
  if (j < j1) {
    const unsigned b = line_begin(d.nl, j), e = d.nl[j];
    const unsigned char *s = (const unsigned char *)d.text;
    ConvertRec r; r.labelOff = 0; r.labelLen = 0; r.chromOff = 0; r.chromLen = 0; r.s0 = 0; r.e = 0; r.outLen = 0; r.strand = '+';
    bool ok = true;
    if (d.format == kConvertFromSam) walk_sam(s, b, e, r);
    else if (d.format == kConvertFromGff) walk_gff(s, b, e, r);
    else {
      gtxtext::LineCols c;
      ok = gtxtext::verbatim_line(s, b, e, c);
      if (!ok) atomicOr(d.flag, 16);
      else {
        r.chromLen = c.nameLen; r.strand = c.strand; r.s0 = (int)c.v2; r.e = (int)c.v3;
        if (c.nTok >= 4) { r.labelOff = c.tailOff + 1; r.labelLen = c.col4End - r.labelOff; }
      }
    }
    if (ok) {
      // -chr: "MT" prints as "chrM" (PrintChromosome :5968-5972) -- the name's first byte
      if (op.to == kConvertBed && op.ucsc && r.chromLen == 2 && s[b + r.chromOff] == 'M' && s[b + r.chromOff + 1] == 'T') r.chromLen = 1;
      r.outLen = out_len(op, r);
    }
    d.rec[j] = r;
    len = r.outLen;
  }
  tile_total(len, &sBytes);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sBytes > (unsigned)kConvertStage) atomicOr(d.flag, 32);
    d.tileBytes[tile] = sBytes;
  }
}

__global__ __launch_bounds__(kConvertTile) void convert_emit_kernel(ConvertDevice d, ConvertOp op)
{
  __shared__ __attribute__((aligned(16))) unsigned char run[kStageBytes];
  __shared__ unsigned waveSum[kConvertTile / 64];
  if (*d.flag) return;
  const unsigned tile = blockIdx.x, j0 = tile * kConvertTile, j1 = min(j0 + kConvertTile, d.nLines);
  const i64 lo = d.baseBytes[tile], hi = d.baseBytes[tile + 1];
  const unsigned j = j0 + threadIdx.x;
  ConvertRec r; r.outLen = 0;
  if (j < j1) r = d.rec[j];
  const unsigned at = tile_exclusive<kConvertTile>(r.outLen, waveSum);   // where the line begins inside the run
  const unsigned pad = (unsigned)(lo & 15);                       // run[k] is byte lo - pad + k of the output; pad + (hi - lo) <= 15 + kConvertStage
  if (r.outLen) {
    const unsigned char *line = (const unsigned char *)d.text + line_begin(d.nl, j);
    const unsigned char *label = line + r.labelOff, *chrom = line + r.chromOff;
    unsigned char *p = run + pad + at;
    auto put_label = [&]() { if (r.labelLen == 0) *p++ = '_'; else for (unsigned k = 0; k < r.labelLen; k++) *p++ = label[k]; };
    if (op.to == kConvertReg) {                                   // LABEL TAB CHROM SP STRAND SP START SP STOP NL
      put_label();
      *p++ = '\t';
      for (unsigned k = 0; k < r.chromLen; k++) *p++ = chrom[k];
      *p++ = ' '; *p++ = (unsigned char)r.strand; *p++ = ' ';
      p = put_signed(p, (i64)r.s0 + 1);
      *p++ = ' ';
      p = put_signed(p, r.e);
    } else {                                                      // CHROM' TAB START-1 TAB STOP TAB LABEL TAB 1000 TAB STRAND [TAB START-1 TAB STOP TAB COLOR] NL
      if (op.ucsc) { *p++ = 'c'; *p++ = 'h'; *p++ = 'r'; }
      for (unsigned k = 0; k < r.chromLen; k++) *p++ = chrom[k];
      *p++ = '\t';
      p = put_signed(p, r.s0);
      *p++ = '\t';
      p = put_signed(p, r.e);
      *p++ = '\t';
      put_label();
      *p++ = '\t'; *p++ = '1'; *p++ = '0'; *p++ = '0'; *p++ = '0'; *p++ = '\t';
      *p++ = (unsigned char)r.strand;
      if (op.colorLen) {
        *p++ = '\t';
        p = put_signed(p, r.s0);
        *p++ = '\t';
        p = put_signed(p, r.e);
        *p++ = '\t';
        for (int k = 0; k < op.colorLen; k++) *p++ = (unsigned char)op.color[k];
      }
    }
    *p++ = '\n';
  }
  __syncthreads();
  store_run<kConvertTile>(d.out, run, lo, (unsigned)(hi - lo));
}

}  // namespace

hipError_t launch_convert(const ConvertDevice &d, const ConvertOp &op, hipStream_t st)
{
  if (d.nLines == 0) return hipSuccess;
  const unsigned nTiles = (unsigned)convert_tiles(d.nLines);
  convert_plan_kernel<<<nTiles, kConvertTile, 0, st>>>(d, op);
  const hipError_t e = launch_tile_prefix(d.tileBytes, (long long)nTiles, d.baseBytes, st);
  if (e != hipSuccess) return e;
  convert_emit_kernel<<<nTiles, kConvertTile, 0, st>>>(d, op);
  return hipGetLastError();
}

}  // namespace gtx
