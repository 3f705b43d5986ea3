// gtx_text.h -- launch interface of the device-side BED / SAM / GFF tokenizer (gtx_text.hip), used by gtx_api_text.hip and gtx_api_link.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "gtx.h"

namespace gtxtext {

struct TextDevice {               // device buffers of one block in flight
  const char *text;               // the block's bytes
  unsigned *segCount;             // [segments + 1] newlines per 1 KB segment, then their exclusive prefix
  unsigned *nl;                   // [n_lines] byte offset of every newline
  int *tri; int *w;               // [n_lines] packed triples / weights
  int *tri2; int *w2; unsigned *blkMinus;   // strand-aware runs: the same grouped by strand ('+' first), and the '-' lines per 128-line block [n_lines / 128 + 2]; null otherwise
  int *flag;                      // != 0: the block is not plain (nothing of it is counted)
  unsigned long long *blockSum, *labelSum;   // scans (may be null): the label values of the block's lines, added to the call's total when the block is plain
};
struct TextTables {               // per reference set: hash table of the chromosome names, the names, the seam's name behind them
  const void *table; unsigned tableMask; const char *names; unsigned prevOff, prevLen;
};
// scanRules: 0 = the overlap algorithms' rules (gtx_text_rules::sorted_rules), 1 = the unsorted scanner's (an interval with start > stop or
// stop <= 0 is skipped silently, genomic_intervals.cpp:5039), 2 = the sorted scanner's (nothing about the interval is checked; order as sorted_rules)
// format: 0 = the lines are BED, 1 = SAM alignments (GTX_TEXT_SAM), 2 = GFF / GTF features (GTX_TEXT_GFF)
hipError_t launch_tokenize(const TextDevice &d, const TextTables &t, const gtx_text_rules &r, size_t bytes, unsigned nLines, hipStream_t st, int scanRules = 0, int format = 0);
// the first step of launch_tokenize on its own, for the passes that read the text themselves (gtx_blocks.h): nl[k] = the offset of
// newline k for k < nLines, segCount [bytes / 1024 + 2] its scratch; segCount[(bytes + 1023) / 1024] = the newlines the text holds
hipError_t launch_newline_index(const char *text, size_t bytes, unsigned *segCount, unsigned *nl, unsigned nLines, hipStream_t st);
void build_tables(const gtx_text_rules &r, std::vector<int32_t> *table, unsigned *mask, std::string *blob);

// ---- gtx_subset_text: the lines of a tokenised block that are kept, byte for byte ----
// A line may be copied instead of printed only if GenomicRegionBED::Print (genomic_intervals.cpp:2188-2218) would render the line
// itself.  On top of the tokenizer's plain case: 3 to 6 tokens, none beginning with or holding a blank, a '\r' or any other byte
// below ' '; columns 2 and 3 canonical decimal ("0" or no leading zero); column 5 a canonical long (optional '-', no leading zero,
// not "-0", at most 18 digits); column 6 exactly "+" or "-".  One line per thread over nl[]; a line that is not raises *flag (16).
// Leaves at once when the tokenizer has already set *flag.
hipError_t launch_verbatim(const char *text, const unsigned *nl, unsigned nLines, int *flag, hipStream_t st);
// line j is kept when (hits[j] == 0) == invert.  tile: 2 * (tiles + 1) words, tiles = subset_tiles(nLines) -- the kept bytes of every
// 256 lines, then the kept lines, each made into its exclusive prefix with the total behind the last; out receives the kept lines
// (newline included) in order.  With *flag set nothing is written but zero totals.
struct SubsetDevice { const char *text; const unsigned *nl; unsigned nLines; const unsigned *hits; int invert; const int *flag; unsigned long long *tile; char *out; };
size_t subset_tiles(unsigned nLines);
hipError_t launch_subset_gather(const SubsetDevice &d, hipStream_t st);

}  // namespace gtxtext
