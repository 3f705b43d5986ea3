// gtx_convert.h -- every line of a tokenised block of SAM, GFF / GTF or BED text printed again as a BED line or as a line of the
// toolkit's REG format, on the device: what `genomic_regions bed` and `genomic_regions reg` print for single-interval regions
// (GenomicRegion::PrintBEDFormat genomic_intervals.cpp:1256-1274, PrintREG :961-971; gtx_convert_text, include/gtx.h).
//
// Count, prefix, emit over tiles of kConvertTile lines, one line per lane, a tile per block; the block's text is on the device with
// its newline index, and launch_tokenize (gtx_text.h) has judged every line plain:
//
//   convert_plan_kernel   a lane walks the head of its line where it lies in global memory, byte by byte, and no further than the
//                         last field it needs: SAM to the end of the CIGAR (QNAME, FLAG, RNAME, POS, the reference length; a CIGAR
//                         of "*" sends it on to SEQ, whose length that CIGAR stands for), GFF to the end of column 9, BED through
//                         verbatim_line (gtx_textline.h), which reads the whole line -- a BED line is its own head.  It records
//                         where label and chromosome lie in the line, the strand, START - 1, STOP and the output length, which
//                         needs digit counts only (ConvertRec).  The tile's bytes go to tileBytes.  (The interval is read here and
//                         not from the tokenizer's triples: without chromosome names, as the block is staged, the tokenizer leaves
//                         class -1 with start and stop 0.)
//   launch_tile_prefix    (gtx_compact.h) exclusive sums of the tiles' bytes.  Every line of a plain block is printed, so the lines
//                         need no prefix of their own
//   convert_emit_kernel   a tile's lines are one run of the output, placed by tile_exclusive and built in LDS: label and chromosome
//                         copied from the text, the decimals rendered, the constant pieces ("\t1000\t", the colour, "chr") put
//                         between them.  The run goes out through store_run (gtx_lineout.h, which has the scheme of the store)
//
// Why the heads are walked in global memory and not staged: the text of 256 SAM lines is 60-150 KB, of which the plan needs some 50
// bytes a line and the emit pass the 10-30 of QNAME and RNAME.  A lane's bytes lie in one or two 128-byte lines, which the vector
// cache keeps for the walk's following loads; staging would bring the other three quarters of the text into LDS to skip them there.
//
// A tile whose run is longer than kConvertStage bytes makes the block not plain (flag 32), as a BED line outside verbatim_line does
// (flag 16): the emit pass writes nothing of such a block and gtx_convert_result reports zero bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gtx {

constexpr int kConvertTile = 256;                 // lines per tile: one per lane of a 256-thread block
constexpr int kConvertStage = 32 * 1024;          // bytes of a tile's run that the LDS stage holds (128 per line on average; four
                                                  // blocks of it share a CU's 160 KiB)
constexpr int kConvertMaxColor = 32;              // bytes of -c the constant piece holds ("255,255,255" is 11)
// What a printed line may be longer than its input line.  With c = the chromosome's and l = the label's bytes, both of which the
// input line holds (so the growth is at most what stands beside them below), and coordinates of at most 10 digits ("-1" is two):
//   bed: 3 ("chr") + c + 1 + 10 + 1 + 10 + 1 + l + 6 ("\t1000\t") + 1 (strand) + 1 (newline)  =  c + l + 34, one more when the
//        label is the "_" of an 8-column GFF line; with a colour 1 + 10 + 1 + 10 + 1 + its bytes on top
//   reg: l + 1 + c + 1 + 1 + 1 + 10 + 1 + 10 + 1  =  c + l + 26, one more for "_"
constexpr int kConvertGrow = 35, kConvertGrowColor = 23;

enum { kConvertBed = 0, kConvertReg = 1 };
enum { kConvertFromBed = 0, kConvertFromSam = 1, kConvertFromGff = 2 };   // launch_tokenize's numbers

struct ConvertOp { int to, ucsc, colorLen; char color[kConvertMaxColor]; };
// labelOff, chromOff: from the line's first byte; labelLen 0: the label is "_".  s0 = START - 1.  outLen: the printed line's bytes
struct ConvertRec { unsigned labelOff, labelLen, chromOff, chromLen; int s0, e; unsigned outLen; int strand; };

struct ConvertDevice {
  const char *text; size_t bytes; const unsigned *nl; unsigned nLines; int format;   // the block as launch_tokenize left it
  int *flag;                                      // the tokenizer's verdict; 16 and 32 are raised here
  ConvertRec *rec;                                // [nLines]
  unsigned *tileBytes;                            // [tiles]
  long long *baseBytes;                           // [tiles + 1]
  char *out;                                      // 16-byte aligned, room for gtx_convert_max_bytes + 32
};

inline size_t convert_tiles(unsigned nLines) { return ((size_t)nLines + kConvertTile - 1) / kConvertTile; }
hipError_t launch_convert(const ConvertDevice &d, const ConvertOp &op, hipStream_t st);

}  // namespace gtx
