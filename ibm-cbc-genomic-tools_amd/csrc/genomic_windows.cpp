// genomic_windows -- MI355X edition of the `win` operation of GenomicTools' genomic_regions (reference driver:
// gtools/genomic_regions.cpp:397-403 operation, :647-651 options, :686-704 the set, :734 the call): every region of a BED set cut into
// sliding windows -- what `bedtools makewindows` does, and what makes the reference set of a binned `genomic_overlaps count`.
//   genomic_windows [-s N] [-d N] [--small] [-v] <REGION-SET>
// Same command line as `genomic_regions win` without the operation word, same output, same errors.  The windows are rendered as
// text on the device (GenomicRegionSet::RunSlidingWindows: gtx_windows_text / gtx_windows_result), i.e. HIP kernels through
// libgtx.so.  genomic_regions keeps refusing the word; this tool is where it lives.
//
// One difference: with -d below 1 the reference's loop does not advance and the run never returns.  This build refuses such a
// distance up front.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_windows";
static const long int BUFFER_SIZE = 10000;

int main(int argc, char *argv[])
{
  GtxAcceptSAM(false);                                        // (the windows print the lines' labels and scores: SAM stays unsupported, as for the tools that print lines)
  bool HELP, HELP2, VERBOSE, WIN_SMALL;
  long WIN_SIZE, WIN_STEP;
  gtxhost::Options opts;                                      // :647-651
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  opts.Long("-s", &WIN_SIZE, 1, "window size");
  opts.Long("-d", &WIN_STEP, 1, "window distance");
  opts.Flag("--small", &WIN_SMALL, "include smaller windows at the end of chromosomes");
  const int next_arg = opts.Parse(argc, argv, 1);
  if (HELP || HELP2) {
    opts.Usage(PROGRAM, "[OPTIONS]", "<REGION-SET>");
    fprintf(stderr, "Creates new invervals by sliding windows.\n\n"
                    "  * Input formats: BED\n  * Operand: region\n  * Region requirements: single-interval\n"
                    "  * Region-set requirements: none\n\n");
    return 1;
  }
  _MESSAGES_ = VERBOSE;
  if (WIN_STEP < 1) { fprintf(stderr, "Error: window distance must be at least 1!\n"); return 1; }

  // :686-704: a file or stdin, streamed, its header echoed
  char *REG_FILE = next_arg == argc ? NULL : argv[next_arg];
  GenomicRegionSet RegSet(REG_FILE, BUFFER_SIZE, VERBOSE, false, false);
  RegSet.RunSlidingWindows(WIN_STEP, WIN_SIZE, WIN_SMALL);
  GtxMark("output written");
  GtxFinish(0);
  return 0;
}
