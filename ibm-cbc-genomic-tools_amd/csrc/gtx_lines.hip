// Kernels of the line renderer (see gtx_lines.h, which has the shape of the passes and the two rules).
#include "gtx_lines.h"

namespace gtx {
namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned uint32x4 __attribute__((ext_vector_type(4)));

__device__ const u64 kPow10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull,
                                   100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                                   100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};

__device__ __forceinline__ int digits(u64 u)
{
  int d = 1;
  while (d < 20 && u >= kPow10[d]) d++;
  return d;
}

// the d digits of u at p
__device__ __forceinline__ void put_digits(char *p, u64 u, int d)
{
  int k = d;
  while (u >> 32) { p[--k] = (char)('0' + (int)(u % 10)); u /= 10; }
  unsigned v = (unsigned)u;
  while (k > 0) { p[--k] = (char)('0' + (int)(v % 10)); v /= 10; }
}

// the last block at or behind b whose offset is at or below `at` (blockOff[b] <= at, or no block's is: then b): a few steps forward,
// then a search
__device__ __forceinline__ int block_of(const i64 *__restrict__ off, int nBlocks, int b, i64 at)
{
  for (int s = 0; s < 4; s++) {
    if (b + 1 < nBlocks && off[b + 1] <= at) b++; else return b;
  }
  int lo = b, hi = nBlocks;
  while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (off[mid] <= at) lo = mid; else hi = mid; }
  return lo;
}

// what a lane keeps of one entry between the test and the write
struct Line { u64 mag; i64 start, stop; int b, vd, sd, ed, nameLen, len; bool neg; };

__device__ __forceinline__ void measure(const LinesLayout &L, int b, i64 at, u64 v, Line &x)
{
  const i64 k = at - L.blockOff[b];
  x.b = b; x.neg = (i64)v < 0; x.mag = x.neg ? 0ull - v : v;
  x.start = L.step * k + 1; x.stop = L.step * k + L.size;
  x.vd = digits(x.mag); x.sd = digits((u64)x.start); x.ed = digits((u64)x.stop);
  x.nameLen = L.nameOff[b + 1] - L.nameOff[b];
  x.len = (x.neg ? 1 : 0) + x.vd + 1 + x.nameLen + 3 + x.sd + 1 + x.ed + 1;
}

__device__ __forceinline__ void put_line(const LinesLayout &L, char *p, const Line &x)
{
  if (x.neg) *p++ = '-';
  put_digits(p, x.mag, x.vd); p += x.vd;
  *p++ = '\t';
  const char *name = L.names + L.nameOff[x.b];
  for (int j = 0; j < x.nameLen; j++) p[j] = name[j];
  p += x.nameLen;
  *p++ = ' '; *p++ = L.strand[x.b]; *p++ = ' ';
  put_digits(p, (u64)x.start, x.sd); p += x.sd;
  *p++ = ' ';
  put_digits(p, (u64)x.stop, x.ed); p += x.ed;
  *p = '\n';
}

__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// PAIRS: the pair rule.  EMIT = false: the tile's kept lines and bytes, the all-ones word.  EMIT = true: the text.
template <bool PAIRS, bool EMIT>
__global__ __launch_bounds__(kLinesThreads) void lines_kernel(LinesArgs a)
{
  extern __shared__ __align__(16) char lds[];
  const LinesLayout &L = a.L;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 tile0 = a.first / kLinesTile;
  const i64 t = (i64)blockIdx.x * (kLinesThreads / 64) + w;
  const i64 tileStart = (tile0 + t) * kLinesTile;
  if (tileStart >= a.end) return;
  const i64 lo = max(tileStart, a.first), hi = min(tileStart + kLinesTile, a.end);
  i64 limit = a.limit;
  i64 tileLo = 0;
  if (EMIT) {
    tileLo = a.baseBytes[t];
    if (a.baseBytes[t + 1] == tileLo) return;                         // no line kept here
    const u64 e = *a.endWord;
    if (e < (u64)limit) limit = (i64)e;
  }
  // the block of the tile's first ordinal
  const i64 firstAt = PAIRS ? a.ordinals[lo] : lo;
  int rowB = 0;
  {
    int l = 0, h = L.nBlocks;                                         // the number of offsets at or below firstAt
    while (l < h) { const int mid = l + ((h - l) >> 1); if (L.blockOff[mid] <= firstAt) l = mid + 1; else h = mid; }
    rowB = l > 0 ? l - 1 : 0;
  }
  char *buf = lds + (size_t)w * lines_wave_lds(L.maxLine);            // (EMIT) buf[0] is byte base16 of the output
  i64 pos = tileLo, base16 = tileLo & ~(i64)15;
  unsigned nLines = 0, nBytes = 0;
  for (int r = 0; r < kLinesRows; r++) {
    const i64 rowStart = tileStart + (i64)r * kLinesRow;
    if (rowStart >= hi) break;
    if (rowStart + kLinesRow <= lo) continue;
    const i64 i = rowStart + 2 * lane;
    const u64x2 v = load_pair(a.values, i, a.end);
    i64 at0 = i, at1 = i + 1;
    if (PAIRS) { const u64x2 o = load_pair((const u64 *)a.ordinals, i, a.end); at0 = (i64)o.x; at1 = (i64)o.y; }
    const bool in0 = i >= lo && i < hi && at0 >= 0 && at0 < limit, in1 = i + 1 >= lo && i + 1 < hi && at1 >= 0 && at1 < limit;
    if (!EMIT) {
      const bool ones0 = in0 && v.x == ~0ull, ones1 = in1 && v.y == ~0ull;
      if (__ballot(ones0 || ones1)) {
        if (ones0) atomicMin(a.endWord, (u64)at0);
        else if (ones1) atomicMin(a.endWord, (u64)at1);
      }
    }
    const bool keep0 = in0 && v.x != ~0ull && (i64)v.x >= a.minValue, keep1 = in1 && v.y != ~0ull && (i64)v.y >= a.minValue;
    const u64 b0 = __ballot(keep0), b1 = __ballot(keep1);
    if ((b0 | b1) == 0) continue;
    // the row's first ordinal is at or below every kept one of the row
    const i64 rowAt = PAIRS ? max(firstAt, (i64)__shfl((long long)at0, 0)) : max(firstAt, rowStart);
    rowB = block_of(L.blockOff, L.nBlocks, rowB, rowAt);
    Line x0, x1;
    x0.len = 0; x1.len = 0;
    int b = rowB;
    // (ordinals that do not ascend are the caller's mistake; a lane then searches from the front, so that k >= 0 and a line stays within maxLine)
    if (keep0) { if (PAIRS && L.blockOff[b] > at0) b = 0; b = block_of(L.blockOff, L.nBlocks, b, at0); measure(L, b, at0, v.x, x0); }
    if (keep1) { if (PAIRS && L.blockOff[b] > at1) b = 0; b = block_of(L.blockOff, L.nBlocks, b, at1); measure(L, b, at1, v.y, x1); }
    const int mine = x0.len + x1.len, incl = gtxscan::wave_inclusive(mine);
    const int rowBytes = __shfl(incl, 63);
    nLines += (unsigned)(__popcll(b0) + __popcll(b1)); nBytes += (unsigned)rowBytes;
    if (EMIT) {
      char *p = buf + (pos - base16) + (incl - mine);
      if (keep0) put_line(L, p, x0);
      if (keep1) put_line(L, p + x0.len, x1);
      wave_sync();
      const i64 newEnd = pos + rowBytes, cEnd = newEnd & ~(i64)15;
      for (i64 c = base16 + 16 * (i64)lane; c + 16 <= cEnd; c += 16 * 64) {
        if (c >= tileLo) *(uint32x4 *)(a.text + c) = *(const uint32x4 *)(buf + (c - base16));
        else for (i64 g = tileLo; g < c + 16; g++) a.text[g] = buf[g - base16];   // the unit shared with the tile in front
      }
      if (cEnd > base16) {                                            // the unfinished unit moves to the front
        const int left = (int)(newEnd - cEnd);
        char keepByte = 0;
        if (lane < left) keepByte = buf[(cEnd - base16) + lane];
        wave_sync();
        if (lane < left) buf[lane] = keepByte;
        base16 = cEnd;
      }
      wave_sync();
      pos = newEnd;
    }
  }
  if (EMIT) {
    const i64 g = max(base16, tileLo) + lane;                          // what is left of the last unit, shared with the tile behind
    if (g < pos) a.text[g] = buf[g - base16];
  } else if (lane == 0) { a.tileLines[t] = nLines; a.tileBytes[t] = nBytes; }
}

template <bool EMIT>
hipError_t launch_lines(const LinesArgs &a, hipStream_t st)
{
  const long long nt = lines_tiles(a.first, a.end);
  if (nt == 0) return hipSuccess;
  const unsigned grid = (unsigned)((nt + kLinesThreads / 64 - 1) / (kLinesThreads / 64));
  const size_t lds = EMIT ? lines_lds_bytes(a.L.maxLine) : 0;
  if (a.ordinals) hipLaunchKernelGGL((lines_kernel<true, EMIT>), dim3(grid), dim3(kLinesThreads), lds, st, a);
  else hipLaunchKernelGGL((lines_kernel<false, EMIT>), dim3(grid), dim3(kLinesThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_lines_count(const LinesArgs &a, hipStream_t st) { return launch_lines<false>(a, st); }
hipError_t launch_lines_emit(const LinesArgs &a, hipStream_t st) { return launch_lines<true>(a, st); }

}  // namespace gtx
