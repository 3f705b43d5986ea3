// gtx_lineout.h -- what the kernels that read a block of text lines and print lines back share: the column rewrite (gtx_rewrite.hip),
// the format conversion (gtx_convert.hip), the sliding windows (gtx_windows.hip) and the block operations (gtx_blocks.hip).  A tile of
// lines, one per lane: its text staged in LDS, its total, the lines' places inside the tile, and the tile's printed run stored from
// LDS.  Device code; the grammars and the renderers stay with their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_scan.h"

namespace gtxline {

typedef unsigned uint32x4 __attribute__((ext_vector_type(4)));

// the first byte of line j of a block whose newlines are at nl[] (a block's bytes lie below 2^32: the entry points refuse more)
__device__ __forceinline__ unsigned line_begin(const unsigned *nl, unsigned j) { return j ? nl[j - 1] + 1 : 0; }

// lds[k] = text[a0 + k] for a0 + k in [a0, t1), by the THREADS threads of the block: a0 is the 16-byte line at or below the first
// byte wanted, whole 16-byte units are loaded as such (so lds is 16-byte aligned and holds t1 - a0 rounded up to 16), and nothing at
// or behind text[bytes] is read.  No barrier: the caller has one between this and its first read of lds.
template <int THREADS>
__device__ __forceinline__ void stage_text(unsigned char *lds, const char *__restrict__ text, size_t bytes, size_t a0, size_t t1)
{
  for (size_t k = (size_t)threadIdx.x * 16; a0 + k < t1; k += (size_t)THREADS * 16) {
    if (a0 + k + 16 <= bytes) *(uint32x4 *)(lds + k) = *(const uint32x4 *)(text + a0 + k);
    else for (size_t q = 0; a0 + k + q < bytes; q++) lds[k + q] = (unsigned char)text[a0 + k + q];
  }
}

// *ldsSum += the sum of v over the block's threads: per wave in registers, then one LDS add per wave.  Every lane of every wave
// calls it.  The caller zeroes *ldsSum with a barrier between that and the call, and has a barrier between the call and its read.
template <class T>
__device__ __forceinline__ void tile_total(T v, T *ldsSum)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(ldsSum, v);
}

// where a line begins inside its tile's run: the block scan of gtx_scan.h, whose one-barrier contract the line kernels rely on
using gtxscan::tile_exclusive;

// Bytes [lo, lo + total) of out from LDS, by the THREADS threads of the block: run[pad + k] is byte lo + k, pad = lo & 15, so run is
// 16-byte aligned and holds 15 + total bytes rounded up to 16; out is 16-byte aligned.  Whole 16-byte units of out go out as such;
// of the first and the last unit, which the run may share with the run in front and the one behind, only the bytes inside
// [lo, lo + total), one by one: nothing outside the run is written.  The caller has a barrier between its last write to run and this.
template <int THREADS>
__device__ __forceinline__ void store_run(char *__restrict__ outAll, const unsigned char *run, long long lo, unsigned total)
{
  const unsigned pad = (unsigned)(lo & 15), end = pad + total;
  char *__restrict__ out = outAll + (lo - pad);
  for (unsigned k = threadIdx.x * 16; k < end; k += THREADS * 16) {
    if (k >= pad && k + 16 <= end) *(uint32x4 *)(out + k) = *(const uint32x4 *)(run + k);
    else for (unsigned q = max(k, pad); q < min(k + 16, end); q++) out[q] = (char)run[q];
  }
}

}  // namespace gtxline
