// genomic_adjacent -- MI355X edition of the `inv`, `gdist` and `test` operations of GenomicTools' genomic_regions (reference driver:
// gtools/genomic_regions.cpp:413-419, :429-435, :445-451 operations, :525-528, :536-538, :627-629 options, :686-704 the set,
// :741-745 the calls): the three operations that compare every region of a position-sorted set with the one directly in front of it.
//   inv    the complement of the set inside the chromosome bounds (`bedtools complement`), one BED line per gap
//   gdist  the distance between successive regions, "label TAB label TAB distance" per pair
//   test   is the file sorted, and how many inclusions and overlaps does it hold (on stderr)
// Same command line behind the operation word, same output, same errors.  The order check, the counts, the distances and the gaps
// come from the device (GenomicRegionSet::RunGlobalInvert / RunGlobalCalcDistances / RunGlobalTest: gtx_gaps, gtx_adjacent), i.e. HIP
// kernels through libgtx.so.  genomic_regions keeps refusing the three words; this tool is where they live.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_adjacent";
static const long int BUFFER_SIZE = 10000;

static void Usage()
{
  fprintf(stderr, "\nUSAGE: \n  %s OPERATION [OPTIONS] <REGION-SET>\n\nOPERATIONS (MI355X path): \n"
                  "  gdist      Computes distances of successive regions.\n"
                  "  inv        Inverts regions given the genome chromosomal boundaries.\n"
                  "  test       Tests whether genomic regions are sorted and non-overlapping.\n\n", PROGRAM);
}

int main(int argc, char *argv[])
{
  GtxAcceptSAM(false);                                        // (inv and gdist print the lines' scores and labels: SAM stays unsupported, as for the tools that print lines)
  if (argc < 2) { Usage(); return 1; }
  const std::string op = argv[1];
  if (op != "gdist" && op != "inv" && op != "test") { fprintf(stderr, "Unknown operation '%s'!\n", op.c_str()); return 1; }

  bool HELP, HELP2, VERBOSE, SORTED_BY_STRAND = false;
  const char *DIST_OP1 = "1", *DIST_OP2 = "1", *GENOME_REG_FILE = "";
  gtxhost::Options opts;
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  const char *about, *needs;
  if (op == "gdist") {                                        // :525-528
    opts.Str("-op1", &DIST_OP1, "1", "reference point of 1st interval in pair (1=start, 2=stop, 5p=5'-end, 3p=3'-end)");
    opts.Str("-op2", &DIST_OP2, "1", "reference point of 2nd interval in pair (1=start, 2=stop, 5p=5'-end, 3p=3'-end)");
    about = "Computes distances of successive regions.";
    needs = "  * Input formats: BED\n  * Operand: region-pair\n  * Region requirements: single-interval\n  * Region-set requirements: sorted by chromosome/strand/start\n\n";
  } else if (op == "inv") {                                   // :536-538
    opts.Str("-g", &GENOME_REG_FILE, "", "genome region-set file");
    about = "Inverts regions given the genome chromosomal boundaries.";
    needs = "  * Input formats: BED\n  * Operand: region-set\n  * Region requirements: single-interval\n  * Region-set requirements: sorted by chromosome/strand/start\n\n";
  } else {                                                    // :627-629
    opts.Flag("-s", &SORTED_BY_STRAND, "input regions are sorted by strand");
    about = "Tests whether genomic regions are sorted and non-overlapping.";
    needs = "  * Input formats: BED\n  * Operand: region\n  * Region requirements: chromosome/strand-compatible, sorted, non-overlapping\n"
            "  * Region-set requirements: sorted by chromosome/(strand)/start\n\n";
  }
  const int next_arg = opts.Parse(argc, argv, 2);
  if (HELP || HELP2) {
    opts.Usage(PROGRAM, op.c_str(), "[OPTIONS] <REGION-SET>");
    fprintf(stderr, "%s\n\n%s", about, needs);
    return 1;
  }
  _MESSAGES_ = VERBOSE;

  // :693 the bounds, then :686-704: a file or stdin, streamed, its header echoed
  StringLIntMap *bounds = op == "inv" ? ReadBounds((char *)GENOME_REG_FILE, VERBOSE) : NULL;
  char *REG_FILE = next_arg == argc ? NULL : argv[next_arg];
  GenomicRegionSet RegSet(REG_FILE, BUFFER_SIZE, VERBOSE, false, false);
  if (op == "gdist") RegSet.RunGlobalCalcDistances((char *)DIST_OP1, (char *)DIST_OP2);
  else if (op == "inv") RegSet.RunGlobalInvert(bounds);
  else RegSet.RunGlobalTest(SORTED_BY_STRAND);
  GtxMark("output written");
  GtxFinish(0);
  return 0;
}
