// Line renderer (gtx_lines_layout / gtx_window_lines* / gtx_pair_lines*, include/gtx.h): the output lines of `genomic_scans counts`
// written as text on the device, from a window vector in HBM or from the (ordinal, value) pairs the window filter left there.  For
// window ordinal `at` in block b of the layout, k = at - blockOff[b], the line is
//
//   VALUE '\t' NAME ' ' ('+'|'-') ' ' step k + 1 ' ' step k + size '\n'
//
// VALUE a signed 64-bit decimal, what GenomicRegionSetScanner::PrintRemaining / PrintFiltered format on the host.  A line's length
// follows from digit counts alone, so the shape is the tile compaction's (gtx_compact.h) with bytes in place of rows:
//
//   lines_kernel<.., false>    per tile of kLinesTile entries the lines kept and their bytes; the smallest ordinal whose value is
//                              all-ones goes into one 64-bit word (atomicMin): the output ends in front of it
//   launch_tile_prefix         twice: exclusive sums of the tiles' lines and of their bytes (64-bit)
//   lines_kernel<.., true>     the rule once more; a wave stages a row's text in LDS at the row's byte prefix inside the tile and
//                              writes it out with 16-byte stores aligned in the output; bytes that share a 16-byte unit with a
//                              neighbouring tile (the tile's head and tail) go out one by one.  A tile without a kept line loads nothing
//
// Two rules over one body.  The vector rule (PrintRemaining): entry i of [first, end) is window i; kept when i < limit and
// (int64) w[i] >= minValue.  The pair rule (PrintFiltered): entry j is (ordinal[j], value[j]), ordinals ascending; kept when
// 0 <= ordinal[j] < limit and (int64) value[j] >= 0.  Under both an all-ones value in front of the limit is never printed and ends
// the output.
//
// A tile belongs to one wave: kLinesRows rows of kLinesRow entries, lane l of a row holding entries 2 l and 2 l + 1 (one 16-byte load
// per vector).  Tiles are cut at multiples of kLinesTile of the ENTRY index, wherever [first, end) begins.  The block of a tile's first
// ordinal is one wave-uniform search over blockOff; a row steps forward from it, a lane from its row's (a few steps, then a search:
// a tile may span more blocks than it has lanes).  No block waits for another and none reads what a block of its own launch wrote.
//
// LDS: a wave stages one row, kLinesRow lines of at most the layout's longest line (maxLine, <= kLinesMaxLine) plus the carry of
// the 16-byte unit the row before left unfinished: lines_lds_bytes(maxLine) per block of four waves.  With names of five letters and
// coordinates of nine digits (maxLine 50) that is 25.1 KiB: six blocks, 24 waves per CU; at the staged name limit (maxLine 112) 56.1 KiB,
// inside the 64 KiB a launch may ask for without an attribute: two blocks, 8 waves per CU.
#pragma once
#include <hip/hip_runtime.h>
#include "gtx_compact.h"

namespace gtx {

constexpr int kLinesThreads = 256, kLinesRows = 8, kLinesRow = 128;
constexpr int kLinesTile = kLinesRow * kLinesRows;                   // entries per wave (include/gtx.h names it: GTX_LINES_TILE)
constexpr int kLinesMaxName = 48;                                    // the longest name a layout may hold (GTX_LINES_MAX_NAME)
// value (sign and 19 digits), tab, name, " s ", start, ' ', stop, '\n'
constexpr int kLinesMaxLine = 20 + 1 + kLinesMaxName + 3 + 19 + 1 + 19 + 1;
static_assert(kLinesTile == kCompactTile, "the line renderer borrows the compaction's tile prefix");

inline long long lines_tiles(long long first, long long end) { return end > first ? (end - 1) / kLinesTile - first / kLinesTile + 1 : 0; }
__host__ __device__ inline size_t lines_wave_lds(int maxLine) { return ((size_t)kLinesRow * maxLine + 32 + 15) & ~(size_t)15; }
inline size_t lines_lds_bytes(int maxLine) { return lines_wave_lds(maxLine) * (kLinesThreads / 64); }

struct LinesLayout {
  const long long *blockOff;                                         // [nBlocks + 1], ascending from 0; the last entry = all windows
  const int *nameOff;                                                // [nBlocks + 1]: block b's name is names[nameOff[b] .. nameOff[b + 1])
  const char *names, *strand;                                        // strand [nBlocks]: '+' or '-'
  int nBlocks, maxLine;
  long long step, size;
};

struct LinesArgs {
  LinesLayout L;
  const unsigned long long *values;                                  // the window vector, or the pairs' values (16-byte aligned)
  const long long *ordinals;                                         // the pair rule's ordinals (16-byte aligned); null under the vector rule
  long long first, end, limit, minValue;
  unsigned *tileLines, *tileBytes;                                   // [tiles]
  const long long *baseBytes;                                        // [tiles + 1] (emit)
  unsigned long long *endWord;                                       // all-ones (~0) = no all-ones value met
  char *text;                                                        // 16-byte aligned (emit)
};

// the count pass over the tiles of [first, end); endWord is left as the call found it or lowered
hipError_t launch_lines_count(const LinesArgs &a, hipStream_t st);
// the emit pass; reads *endWord: what lies at or behind that ordinal is not rendered
hipError_t launch_lines_emit(const LinesArgs &a, hipStream_t st);

}  // namespace gtx
