// gtx_rewrite.h -- columns 2 and 3 of every line of a tokenised block of BED text rewritten on the device, lines dropped, everything
// else kept byte for byte: what `genomic_regions shift | shiftp | pos | center | fix | bounds` print (gtx_rewrite_text, include/gtx.h).
//
// Count, prefix, emit over tiles of kRewriteTile lines, one line per lane, a tile per block; the block's text is on the device with
// its newline index and the tokenizer's triples (launch_tokenize, gtx_text.h):
//
//   rewrite_plan_kernel   the tile's text staged in LDS (stage_text, gtx_lineout.h).  A lane walks its line with the predicate the
//                         subset's gather uses (verbatim_line, gtx_textline.h: the line is plain), which hands it columns 2, 3 and 6,
//                         applies the operation in signed 64-bit arithmetic and records kept / dropped, s' - 1, e', the length of
//                         column 1, where the tail begins and the output length (RewriteRec).  The tile's bytes and lines go to
//                         tileBytes / tileLines.  `bounds` takes the chromosome from the tokenizer's class of the line (its hash
//                         table of the names); the other operations never look at the name
//   launch_tile_prefix    (gtx_compact.h) twice: exclusive sums of the tiles' bytes and lines
//   rewrite_emit_kernel   a tile's kept lines are one run of the output.  The tile's text is staged again, the lines are placed
//                         (tile_exclusive), the run is built in LDS -- column 1 copied, two signed decimals rendered, the tail
//                         copied with its newline -- and goes out through store_run (gtx_lineout.h, which has the scheme of the
//                         store).  A tile without a kept line returns before it loads anything
//
// A tile whose text, or whose run, is longer than kRewriteStage bytes makes the block not plain (flag 32), as a line outside the
// predicate does (flag 16): the emit pass writes nothing of such a block.  (The prefixes still sum the tiles that were planned;
// gtx_rewrite_result looks at the flag first and reports zero bytes and lines.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gtx {

constexpr int kRewriteTile = 256;                 // lines per tile: one per lane of a 256-thread block
constexpr int kRewriteStage = 24 * 1024;          // bytes of a tile's text, and of its run, that the LDS stages hold (96 per line on
                                                  // average; two stages of it leave room for three blocks on a CU's 160 KiB)
constexpr int kRewriteGrow = 38;                  // a line grows by at most two signed 64-bit decimals (20 bytes each) in place of two digits

enum { kRewriteShift = 0, kRewriteShiftP = 1, kRewritePos = 2, kRewriteCenter = 3, kRewriteFix = 4, kRewriteBounds = 5 };
enum { kPosStart = 0, kPosStop = 1, kPos5p = 2, kPos3p = 3, kPosCenter = 4 };

struct RewriteOp { int kind, posOp; long long a, b; const long long *chromLen; int nChrom; };   // chromLen: device memory, per class of the tokenizer
struct RewriteRec { long long s0, e1; unsigned nameLen, tailOff, outLen, pad; };                 // outLen 0: the line is dropped

struct RewriteDevice {
  const char *text; size_t bytes; const unsigned *nl; unsigned nLines; const int *tri;   // the block as launch_tokenize left it
  int *flag;                                      // the tokenizer's verdict; 16 and 32 are raised here
  RewriteRec *rec;                                // [nLines]
  unsigned *tileBytes, *tileLines;                // [tiles]
  long long *baseBytes, *baseLines;               // [tiles + 1]
  char *out;                                      // 16-byte aligned, room for bytes + kRewriteGrow * nLines
};

inline size_t rewrite_tiles(unsigned nLines) { return ((size_t)nLines + kRewriteTile - 1) / kRewriteTile; }
hipError_t launch_rewrite(const RewriteDevice &d, const RewriteOp &op, hipStream_t st);

}  // namespace gtx
