// gtx_textline.h -- the one predicate "GenomicRegionBED::Print would render this line as it stands" (see gtx_text.h), for the
// kernels that write text out from text in: the subset's gather (gtx_text.hip), the column rewrite (gtx_rewrite.hip), the sliding
// windows (gtx_windows.hip) and the format conversion of BED lines (gtx_convert.hip); and the decimals (digits, signed_len,
// put_signed) that the last three and the block operations (gtx_blocks.hip, which has a grammar of its own) render.  What these
// kernels share of a tile's staging, scan and store is in gtx_lineout.h.  Device code.
#pragma once
#include <hip/hip_runtime.h>

namespace gtxtext {

// the decimal digits of u
__device__ __forceinline__ int digits(unsigned long long u)
{
  int d = 1;
  for (unsigned long long p = 10; d < 20 && u >= p; p *= 10) d++;
  return d;
}
__device__ __forceinline__ int signed_len(long long v) { return v < 0 ? 1 + digits(0ull - (unsigned long long)v) : digits((unsigned long long)v); }

// "%ld" of v at p; returns the byte behind it
__device__ __forceinline__ unsigned char *put_signed(unsigned char *p, long long v)
{
  unsigned long long u = (unsigned long long)v;
  if (v < 0) { *p++ = '-'; u = 0ull - u; }
  const int d = digits(u);
  int k = d;
  while (u >> 32) { p[--k] = (unsigned char)('0' + (int)(u % 10)); u /= 10; }
  unsigned w = (unsigned)u;
  while (k > 0) { p[--k] = (unsigned char)('0' + (int)(w % 10)); w /= 10; }
  return p + d;
}

// what the walk over a verbatim line has seen of it: the length of column 1, where the tail begins (the byte behind column 3, a tab
// or the line's end, as an offset from the line's first byte), columns 2 and 3 as numbers, the number of tokens and the strand of
// column 6 ('+' with fewer than 6 columns, genomic_intervals.cpp:2165), and the byte behind column 4 as such an offset (0 with 3 columns)
struct LineCols { unsigned nameLen, tailOff; long long v2, v3; int nTok, strand; unsigned col4End; };

// does Print re-render the line [b, e) of s as it stands?  (gtx_text.h has the conditions.)  cols is filled as far as the walk got.
template <class PTR>
__device__ __forceinline__ bool verbatim_line(PTR s, unsigned b, unsigned e, LineCols &cols)
{
  int tok = 1;
  unsigned q = b;                                                 // the token's first byte
  cols.nameLen = 0; cols.tailOff = 0; cols.v2 = 0; cols.v3 = 0; cols.nTok = 0; cols.strand = '+'; cols.col4End = 0;
  for (unsigned p = b;; p++) {
    if (p < e && s[p] != '\t') { if (s[p] <= ' ') return false; continue; }
    const unsigned n = p - q;
    if (n == 0 || tok > 6) return false;
    if (tok == 1) cols.nameLen = n;
    else if (tok == 2 || tok == 3) {
      unsigned long long v = 0;
      for (unsigned k = q; k < p; k++) { if ((unsigned)(s[k] - '0') >= 10u) return false; v = v * 10 + (unsigned)(s[k] - '0'); }
      if (n > 1 && s[q] == '0') return false;
      if (tok == 2) cols.v2 = (long long)v; else { cols.v3 = (long long)v; cols.tailOff = p - b; }
    } else if (tok == 4) cols.col4End = p - b;
    else if (tok == 5) {
      const bool neg = s[q] == '-';
      const unsigned r = q + (neg ? 1 : 0), nd = p - r;
      if (nd == 0 || nd > 18) return false;
      for (unsigned k = r; k < p; k++) if ((unsigned)(s[k] - '0') >= 10u) return false;
      if (s[r] == '0' && (nd > 1 || neg)) return false;
    } else if (tok == 6) {
      if (n != 1 || (s[q] != '+' && s[q] != '-')) return false;
      cols.strand = s[q];
    }
    if (p >= e) break;
    tok++; q = p + 1;
  }
  cols.nTok = tok;
  return tok >= 3;
}

}  // namespace gtxtext
