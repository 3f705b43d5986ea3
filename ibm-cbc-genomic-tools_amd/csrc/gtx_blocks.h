// gtx_blocks.h -- the per-region operations of genomic_regions that look inside a BED12 line, on the device: split, connect, select,
// diff, n and strand (GenomicRegionBED::RunSplit genomic_intervals.cpp:2502-2505 over PrintModified :2310-2314; GenomicRegion::Connect
// :1319-1339, Select :1493-1521, Diff :1345-1361, RunSize :1451-1454, ModifyStrand :1607-1620; UpdateThick :2326-2333 and
// GenomicRegionBED::Print :2188-2218; gtx_blocks_text, include/gtx.h, which has the grammar of the plain line).
//
// The tokenizer (gtx_text.h) calls a 12-column line not plain, so nothing here starts from its verdict or its triples: the passes
// need the block's text and its newline index (launch_newline_index) only.  Count, prefix, emit:
//
//   blocks_plan_kernel    one line per lane, kBlocksTile lines per block.  The lane walks its line once where it lies in global
//                         memory and checks the plain line's grammar on the way: the columns, then the two lists in step, from which
//                         it takes the first and the last block, the sum of the sizes, the gaps between successive blocks (their
//                         number, the first one's start, the last one's stop) and the digits the operation's fresh lists will take.
//                         Nothing is rendered; the printed bytes follow from digit counts and the lengths of the copied columns
//                         (BlocksRec).  A line that prints nothing (select without a flag, diff of a single block or of touching
//                         blocks) has outLen 0 and is counted out.  The tile's bytes and printed lines go to tileBytes / tileCount
//   launch_tile_prefix    (gtx_compact.h) exclusive sums of both; the totals are the block's bytes and n_printed
//   blocks_emit_kernel    connect, select, diff, n, strand: a tile's printed lines are one run of the output, placed by
//                         tile_exclusive over the tile's one wave, built in LDS and stored through store_run (gtx_lineout.h, which
//                         has the scheme of the store).  A record cannot hold a block
//                         list: diff walks the two lists again, strand copies them.  A tile whose run is longer than kBlocksStage
//                         makes the block not plain (flag 32, raised by the plan)
//   blocks_base_kernel,   split prints blocks x (chromosome + label + about 45) bytes per line, far beyond any stage for a tile of
//   blocks_split_kernel   lines, so its emit is driven by the output: the lines' exclusive sums of printed lines and bytes (lineOut,
//                         lineByte), then one lane per printed line, kBlocksOutTile of them per block wherever in the input they
//                         lie.  A lane finds its input line by a search in lineOut and its block by walking the lists to its ordinal,
//                         summing the bytes of the blocks in front on the way.  The block's lines are one run, staged and stored as
//                         above; a run longer than kBlocksOutStage (labels of hundreds of bytes) is stored by its lanes directly,
//                         byte by byte, so that no split block comes back for its size
//
// Why the lines are walked in global memory and not staged in LDS: a BED12 line is 60 bytes for a spliced read and 8 KB for a
// transcript of 363 exons, so the text of a tile has no bound that a stage could be sized for, and a second reason to send a block
// back would come with it.  A lane's walk is sequential; its bytes lie in consecutive 128-byte lines which the vector cache keeps
// for the loads that follow.
//
// kBlocksTile x kBlocksStage: 64 lines whose output may be 48 KiB, i.e. 768 bytes a line on average against the 150 to 250 of a
// ten-exon transcript; a 363-exon transcript prints about 4 KB of lists, so a tile holds ten of them side by side.  Three such
// blocks share a CU's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gtx {

constexpr int kBlocksTile = 64;                   // lines per tile of the plan and of the one-line emit: one per lane of a wave
constexpr int kBlocksStage = 48 * 1024;           // bytes of a tile's run that the LDS stage holds
constexpr int kBlocksMax = 1024;                  // blocks of a plain line (column 10)
constexpr int kBlocksOutTile = 256;               // split: printed lines per emit block
constexpr int kBlocksOutStage = 32 * 1024;        // split: bytes of an emit block's run that the LDS stage holds
constexpr unsigned kBlocksLineMax = 1u << 25;     // printed bytes of one input line (a tile's sum stays inside 32 bits)
constexpr long long kBlocksLimit = 2147483646ll;  // coordinates lie below it, as the tokenizer's do

enum { kBlocksSplit = 0, kBlocksConnect = 1, kBlocksSelect = 2, kBlocksDiff = 3, kBlocksSize = 4, kBlocksStrand = 5 };
enum { kBlocksFirst = 1, kBlocksLast = 2, kBlocks5p = 4, kBlocks3p = 8 };
enum { kBlocksPlus = 0, kBlocksMinus = 1, kBlocksReverse = 2 };

struct BlocksOp { int kind, select, strandOp; };

// What the plan keeps of a line.  Offsets count from the line's first byte.  nTok: 3 to 6, or 12.  labelLen 0: the label is "_";
// scoreLen 0: the score is "0".  s0 = START - 1 (column 2), e = STOP (column 3), t0 / t1 columns 7 and 8.  Of a 12-column line: n
// blocks; the sizes at [sizesOff, sizesEnd) and the starts at [startsOff, startsEnd), a trailing comma left out; sz0 the first
// block's size, stL the last block's start; sum of the sizes; gaps between successive blocks: their number, gA = where the first
// begins and gZ = where the last ends (both relative to s0, 0-based start / 1-based stop as BED writes them); listDigits: the
// digits of the fresh lists (split: of every printed START - 1 and STOP; diff: of the gaps' sizes and relative starts).
// outLen / outCount: the bytes and lines the operation prints for the line.
struct BlocksRec {
  unsigned nTok, lineLen, nameLen, labelOff, labelLen, scoreOff, scoreLen, strandOff, rgbOff, rgbLen;
  unsigned sizesOff, sizesEnd, startsOff, startsEnd;
  unsigned n, sz0, stL, sum, gaps, gA, gZ, listDigits;
  int s0, e, t0, t1, strand;
  unsigned outLen, outCount;
};

struct BlocksDevice {
  const char *text; size_t bytes; const unsigned *nl; const unsigned *nlTotal; unsigned nLines;   // the block and its newline index; *nlTotal: the newlines found
  int *flag;                                      // != 0: the block is not plain.  1: the index, 16: a line, 32: a tile's run
  BlocksRec *rec;                                 // [nLines]
  unsigned *tileBytes, *tileCount;                // [tiles]
  long long *baseBytes, *baseCount;               // [tiles + 1]
  unsigned *lineOut; long long *lineByte;         // split: [nLines + 1]
};

inline size_t blocks_tiles(unsigned nLines) { return ((size_t)nLines + kBlocksTile - 1) / kBlocksTile; }
// plan, the two prefixes and, for split, the lines' bases: baseBytes[tiles] and baseCount[tiles] are the block's totals
hipError_t launch_blocks_plan(const BlocksDevice &d, const BlocksOp &op, hipStream_t st);
// the printed text into out (16-byte aligned, room for totalBytes + 32); totalLines: baseCount[tiles].  Nothing is written when *flag is set
hipError_t launch_blocks_emit(const BlocksDevice &d, const BlocksOp &op, long long totalLines, char *out, hipStream_t st);

}  // namespace gtx
