// genomic_blocks -- MI355X edition of the six operations of GenomicTools' genomic_regions that look inside a region's intervals, which
// for BED input means inside a 12-column line: a transcript with its exons, a spliced read of `bamToBed -bed12` (reference driver:
// gtools/genomic_regions.cpp:237-251, :285-291, :325-331, :365-387 operations, :509-514, :551-553, :600-605, :617-623 options, :702-704
// the set with its header shown, :715-716, :721, :728, :732-733 the calls):
//   split      every interval of a region on a line of its own (bed12ToBed6)
//   connect    the region from its least start to its greatest stop (the gene span)
//   select     the first or last interval, or the one at the 5' or 3' end
//   diff       the gaps between successive intervals (introns)
//   n          the sum of the intervals' lengths (the spliced length)
//   strand     the strand set or reversed
// Same command line behind the operation word, same output, same errors; BED input only.  Plain lines are printed on the device
// (GenomicRegionSet::RunSplit, RunConnect, RunSelect, RunDiff, RunSize, RunModifyStrand: gtx_blocks_text / gtx_blocks_result), i.e.
// HIP kernels through libgtx.so.  genomic_regions keeps refusing the six words; this tool is where they live.
//
// One difference: `strand -s`, the reference's temp-file merge of a sorted set (genomic_intervals.cpp:4365-4390), is not offered.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_blocks";
static const long int BUFFER_SIZE = 10000;

static void Usage()
{
  fprintf(stderr, "\nUSAGE: \n  %s OPERATION [OPTIONS] <REGION-SET>\n\nOPERATIONS (MI355X path): \n"
                  "  connect    Connects intervals from minimum start to maximum stop position.\n"
                  "  diff       Computes the difference between successive intervals.\n"
                  "  n          Computes sum of lengths of intervals in a region (including possible overlaps).\n"
                  "  select     Selects a subset of intervals according to their position in the region.\n"
                  "  split      Splits regions into their intervals which are printed on separate lines.\n"
                  "  strand     Modifies interval strand information.\n\n", PROGRAM);
}

int main(int argc, char *argv[])
{
  GtxAcceptSAM(false);
  if (argc < 2) { Usage(); return 1; }
  const std::string op = argv[1];
  if (op != "split" && op != "connect" && op != "select" && op != "diff" && op != "n" && op != "strand") { fprintf(stderr, "Unknown operation '%s'!\n", op.c_str()); return 1; }

  bool HELP, HELP2, VERBOSE, SELECT_FIRST = false, SELECT_LAST = false, SELECT_5P = false, SELECT_3P = false, SPLIT_BY_CHROM_AND_STRAND = false;
  const char *STRAND_OP = "+";
  gtxhost::Options opts;
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  const char *about, *needs;
  if (op == "connect") {                                      // :237-243, :509-511
    about = "Connects intervals from minimum start to maximum stop position.";
    needs = "  * Input formats: BED\n  * Operand: region\n  * Region requirements: chromosome/strand-compatible\n  * Region-set requirements: none\n\n";
  } else if (op == "diff") {                                  // :245-251, :512-514
    about = "Computes the difference between successive intervals.";
    needs = "  * Input formats: BED\n  * Operand: interval pair\n  * Region requirements: chromosome/strand-compatible, sorted, non-overlapping\n"
            "  * Region-set requirements: none\n\n";
  } else if (op == "n") {                                     // :285-291, :551-553
    about = "Computes sum of lengths of intervals in a region (including possible overlaps).";
    needs = "  * Input formats: BED\n  * Operand: region\n  * Region requirements: none\n  * Region-set requirements: none\n\n";
  } else if (op == "select") {                                // :325-331, :600-605
    opts.Flag("-first", &SELECT_FIRST, "select the first interval");
    opts.Flag("-last", &SELECT_LAST, "select the last interval");
    opts.Flag("-5p", &SELECT_5P, "select the first from the 5' end");
    opts.Flag("-3p", &SELECT_3P, "select the first from the 3' end");
    about = "Selects a subset of intervals according to their position in the region.";
    needs = "  * Input formats: BED\n  * Operand: region\n  * Region requirements: chromosome/strand-compatible\n  * Region-set requirements: none\n\n";
  } else if (op == "split") {                                 // :365-371, :617-619
    opts.Flag("--by-chrstrand", &SPLIT_BY_CHROM_AND_STRAND, "sort and split by chromosome and strand (REG format only)");
    about = "Splits regions into their intervals which are printed on separate lines.";
    needs = "  * Input formats: BED\n  * Operand: region\n  * Region requirements: none\n  * Region-set requirements: none\n\n";
  } else {                                                    // :373-379, :620-623 (without -s)
    opts.Str("-op", &STRAND_OP, "+", "strand operation (+=positive, -=negative, r=reverse)");
    about = "Modifies interval strand information.";
    needs = "  * Input formats: BED\n  * Operand: interval\n  * Region requirements: chromosome/strand-compatible\n  * Region-set requirements: none\n\n";
  }
  const int next_arg = opts.Parse(argc, argv, 2);
  if (HELP || HELP2) {
    opts.Usage(PROGRAM, op.c_str(), "[OPTIONS] <REGION-SET>");
    fprintf(stderr, "%s\n\n%s", about, needs);
    return 1;
  }
  _MESSAGES_ = VERBOSE;

  // :686-704: a file or stdin, streamed, its header lines echoed (:702-704)
  char *REG_FILE = next_arg == argc ? NULL : argv[next_arg];
  GenomicRegionSet RegSet(REG_FILE, BUFFER_SIZE, VERBOSE, false, false);
  if (RegSet.n_regions > 0 && RegSet.format != "BED") { fprintf(stderr, "Error: the block operations take BED input!\n"); GtxFinish(1); return 1; }
  if (op == "split") RegSet.RunSplit(SPLIT_BY_CHROM_AND_STRAND);
  else if (op == "connect") RegSet.RunConnect();
  else if (op == "select") RegSet.RunSelect(SELECT_FIRST, SELECT_LAST, SELECT_5P, SELECT_3P);
  else if (op == "diff") RegSet.RunDiff();
  else if (op == "n") RegSet.RunSize();
  else RegSet.RunModifyStrand(STRAND_OP);
  GtxMark("output written");
  GtxFinish(0);
  return 0;
}
