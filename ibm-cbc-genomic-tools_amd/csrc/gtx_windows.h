// gtx_windows.h -- every line of a tokenised block of BED text cut into sliding windows on the device: what `genomic_regions win`
// prints (gtx_windows_text / gtx_windows_result, include/gtx.h; GenomicRegionBED::PrintWindows genomic_intervals.cpp:2520-2532).
//
// A line of columns CHROM, v2, v3 [, LABEL [, SCORE [, STRAND]]] has START = v2 + 1, STOP = v3, len = v3 - v2 and, for a window
// size and step >= 1,
//
//   c = 0 when size > len (len <= 0 included), else (len - size) / step + 1      the windows of full size
//   n = c without --small; with it 0 when len <= 0, else (len - 1) / step + 1     the windows printed
//   window k:  CHROM '\t' v2 + k step '\t' (k < c ? v2 + size + k step : STOP) TAIL '\n'
//
// TAIL is "\tLABEL" for 4 or 5 columns (the score of a 5-column line is dropped), the line's own bytes behind column 3 for 6, and
// nothing for 3.  Both numbers run through arithmetic progressions, so the bytes of the first k windows of a line are a closed form
// of digit counts (progression_digits below): nothing loops over the windows in front of a window.  The output's size has nothing to
// do with the input's -- one chromosome line is a hundred million windows, a read two or three -- so the passes are input-driven as
// far as the plan goes and output-driven from there:
//
//   windows_plan_kernel    tiles of kWindowsLineTile lines, one per lane, the tile's text staged in LDS (stage_text, gtx_lineout.h:
//                          the column rewrite's shape).  verbatim_line (gtx_textline.h) decides whether a line is plain; a plain line's record
//                          (WindowsRec) holds n, c, v2, STOP, where its name and tail lie in the block's text and how long they are.
//                          The tile's windows and bytes go to tileWindows / tileBytes, 64-bit both: one line can exceed 2^32 in either
//   launch_tile_prefix64   (gtx_compact.h) twice: exclusive sums of the tiles' windows and bytes
//   windows_base_kernel    a tile's lines once more: lineWin[j], lineByte[j] = the windows and bytes in front of line j in the block
//                          (the tile's base plus tile_exclusive over its 256 lines, both sums in one scan); entry nLines holds
//                          the totals
//   windows_emit_kernel    one block of threads per output tile of kWindowsOutTile consecutive window ordinals of the block of text,
//                          over a range of such tiles (the caller streams ranges, gtx_windows_result).  The block finds the line of
//                          its first ordinal by a search over lineWin, 64 probes a step, and holds the bases of the kWindowsSpan
//                          lines from there on in LDS, which as a rule reach the line of its last ordinal; each lane finds the line
//                          and the k of its windows there (else in global memory, between the first line and the last), their
//                          byte offsets from lineByte and the closed form, and renders them
//                          into the tile's run in LDS: name and tail from the block's text, the numbers with put_signed.  The run
//                          goes out through store_run (gtx_lineout.h), at its place in the range's buffer.
//                          A tile may lie inside one line, hold part of a line and hundreds of short ones, or cross any number of
//                          line tiles (lines without a window take no room in it): all the same to the search
//
// A line whose fixed part -- column 1, two tabs, the tail, the newline -- is longer than kWindowsMaxFixed makes the block not plain
// (flag 32), as a tile of lines whose text is longer than kWindowsStage does and as a line outside the predicate does (flag 16): an
// output tile's run is then at most kWindowsRunBytes and fits its stage.  Nothing is emitted of such a block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gtx {

constexpr int kWindowsLineTile = 256;             // lines per tile of the plan: one per lane of a 256-thread block
constexpr int kWindowsStage = 24 * 1024;          // bytes of a line tile's text that the plan's LDS stage holds
constexpr int kWindowsThreads = 256, kWindowsPerLane = 2;
constexpr int kWindowsOutTile = kWindowsThreads * kWindowsPerLane;   // window ordinals per output tile
constexpr int kWindowsMaxFixed = 64;              // bytes of a line's fixed part
constexpr int kWindowsMaxLine = kWindowsMaxFixed + 20;               // ... and two numbers of at most 10 digits
constexpr int kWindowsRunBytes = kWindowsOutTile * kWindowsMaxLine;  // the bound of an output tile's run (42 KiB)
constexpr int kWindowsSpan = 1024;                // lines whose bases an emit block holds in LDS

struct WindowsOp { long long size, step; int small; };
struct WindowsRec {
  long long n, c, bytes;                          // windows printed; those of full size; the bytes of the n
  int v2, stop;                                   // column 2; STOP (below 2^31 - 2 on a plain line)
  unsigned nameOff, tailOff;                      // offsets into the block's text
  unsigned short nameLen, tailLen;                // tailLen: with its leading tab, without the newline
  unsigned pad;
};

struct WindowsDevice {
  const char *text; size_t bytes; const unsigned *nl; unsigned nLines;   // the block as launch_tokenize left it
  int *flag;                                      // the tokenizer's verdict; 16 and 32 are raised here
  WindowsRec *rec;                                // [nLines]
  unsigned long long *tileWindows, *tileBytes;    // [tiles]
  long long *baseWindows, *baseBytes;             // [tiles + 1]
  long long *lineWin, *lineByte;                  // [nLines + 1]
};

// a range [first, first + tiles * kWindowsOutTile) of window ordinals (cut at the block's total) into out (16-byte aligned, room for
// tiles * kWindowsRunBytes + 16); base = the bytes of the windows in front of `first`, which the caller knows from the ranges in
// front (0 for first = 0); total = the block's windows, which the caller has with the plan's verdict: the emit pass reads neither and
// must not be launched on a block whose flag is set.  *rangeBytes = the bytes written.  first + (tiles - 1) * kWindowsOutTile lies in
// front of the total
struct WindowsRange { long long first, tiles, base, total; char *out; unsigned long long *rangeBytes; };

inline size_t windows_tiles(unsigned nLines) { return ((size_t)nLines + kWindowsLineTile - 1) / kWindowsLineTile; }
// plan, the two prefixes, the lines' bases
hipError_t launch_windows_plan(const WindowsDevice &d, const WindowsOp &op, hipStream_t st);
hipError_t launch_windows_emit(const WindowsDevice &d, const WindowsOp &op, const WindowsRange &r, hipStream_t st);

}  // namespace gtx
