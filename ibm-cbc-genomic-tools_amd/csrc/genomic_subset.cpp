// genomic_subset -- MI355X edition of the `subset` operation of GenomicTools' genomic_overlaps (reference driver:
// gtools/genomic_overlaps.cpp:185-191 and :246-249 options, :298-305, :782-800 subset): prints the test regions that overlap some
// reference region, with -inv those that overlap none.  Same command line behind the operation word, same output, same errors.
// The hits of every test region come from the device (GtxPrintSubset: gtx_query_hits, or the file's text selected there by
// gtx_subset_text), i.e. HIP kernels through libgtx.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_subset";
static const long int BUFFER_SIZE = 10000;

int main(int argc, char *argv[])
{
  GtxAcceptSAM(false);                                        // (the selected lines are printed in their own format: SAM stays unsupported, as for overlap)
  bool HELP, HELP2, VERBOSE, IS_SORTED, SORTED_BY_STRAND, IGNORE_STRAND, MATCH_GAPS, SUBSET_NONOVERLAPS;
  const char *BIN_BITS;
  gtxhost::Options opts;
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  opts.Str("-B", &BIN_BITS, "17,20,23,26", "number of shift-bits for each bin level (accepted, unused: no output depends on the order of the matches)");
  opts.Flag("-S", &IS_SORTED, "test and reference regions are sorted by chromosome and start position");
  opts.Flag("-s", &SORTED_BY_STRAND, "test and reference regions are also sorted by strand (-S must be set)");
  opts.Flag("-i", &IGNORE_STRAND, "ignore strand while finding overlaps");
  opts.Flag("-gaps", &MATCH_GAPS, "matching gaps between intervals are considered overlaps");
  opts.Flag("-inv", &SUBSET_NONOVERLAPS, "print test regions that do *not* overlap with reference regions");
  int next_arg = opts.Parse(argc, argv, 1);
  if (HELP || HELP2 || argc - next_arg < 1) { opts.Usage(PROGRAM, "[OPTIONS]", "REFERENCE-REGION-FILE <TEST-REGION-FILE>"); return 1; }
  _MESSAGES_ = VERBOSE;

  if (IS_SORTED && SORTED_BY_STRAND && IGNORE_STRAND) {
    fprintf(stderr, "[Error]: the input is sorted by chromosome/strand/start (i.e. -S and -s are set), therefore the overlap algorithm can only report strand-specific results (i.e. -i cannot be set)!\n");
    return 1;
  }

  // :786-787: the test set is streamed with its header echoed; the index set is loaded in memory, under -S too (as overlap does here)
  char *REF_REG_FILE = argv[next_arg];
  char *TEST_REG_FILE = next_arg + 1 == argc ? NULL : argv[next_arg + 1];
  GenomicRegionSet RefRegSet(REF_REG_FILE, BUFFER_SIZE, VERBOSE, true, true);
  GenomicRegionSet TestRegSet(TEST_REG_FILE, BUFFER_SIZE, VERBOSE, false, false);
  GenomicRegionSetOverlaps *overlaps;
  if (IS_SORTED) overlaps = new SortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, SORTED_BY_STRAND);
  else overlaps = new UnsortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, BIN_BITS);
  GtxPrintSubset(overlaps, MATCH_GAPS, IGNORE_STRAND, SUBSET_NONOVERLAPS, BIN_BITS);
  GtxMark("output written");
  GtxFinish(0);
  delete overlaps;
  return 0;
}
