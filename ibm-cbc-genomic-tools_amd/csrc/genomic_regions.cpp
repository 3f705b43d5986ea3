// genomic_regions -- MI355X edition of the `link` operation of GenomicTools' genomic_regions (reference driver:
// gtools/genomic_regions.cpp:437-451 operation, :469-471 and :546-550 options, :686-704 the set, :744 the call): a position-sorted
// region set merged into its covered territory, one "label TAB chromosome strand start stop" line per group -- what `bedtools merge`
// does.  Same command line behind the operation word, same output, same errors.  The group boundaries, the groups' stops and the
// integer label folds come from the device (GenomicRegionSet::RunGlobalLink: gtx_link), i.e. HIP kernels through libgtx.so.
//
// The reference's other operations are outside this build and are refused by name.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_regions";
static const long int BUFFER_SIZE = 10000;

// the operation words of the reference (genomic_regions.cpp:189-451)
static const char *OTHER_OPERATIONS[] = {"align", "annotator", "bed", "bounds", "center", "chrom", "connect", "diff", "dist", "divide", "fix", "int", "n", "pos",
                                         "reg", "rnd", "search", "select", "shift", "shiftp", "shuffle", "sort", "split", "strand", "union", "wig", "win", "x",
                                         "gdist", "gsort", "inv", "test", NULL};

int main(int argc, char *argv[])
{
  GtxAcceptSAM(false);                                        // (the groups print the head's label: SAM stays unsupported, as for the tools that print lines)
  if (argc < 2) {
    fprintf(stderr, "\nUSAGE: \n  %s OPERATION [OPTIONS] <REGION-SET>\n\nOPERATIONS (MI355X path): \n"
                    "  link       Links consecutive regions to produce a non-overlapping set.\n\n", PROGRAM);
    return 1;
  }
  const std::string op = argv[1];
  for (const char **o = OTHER_OPERATIONS; *o; o++)
    if (op == *o) { fprintf(stderr, "Operation '%s' is outside the MI355X path of this build!\n", *o); return 1; }
  if (op != "link") { fprintf(stderr, "Unknown operation '%s'!\n", op.c_str()); return 1; }

  bool HELP, HELP2, VERBOSE, SORTED_BY_STRAND;
  long LINK_MAX_DIFFERENCE;
  const char *LINK_LABEL_FUNC;
  gtxhost::Options opts;                                      // :469-471, :546-550
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  opts.Flag("-s", &SORTED_BY_STRAND, "input regions are sorted by strand");
  opts.Long("-d", &LINK_MAX_DIFFERENCE, 0, "maximum difference between successive regions");
  opts.Str("--label-func", &LINK_LABEL_FUNC, "", "label function = {min,max,sum,%c}, where %c is used as delimiter");
  const int next_arg = opts.Parse(argc, argv, 2);
  if (HELP || HELP2) {
    opts.Usage(PROGRAM, "link", "[OPTIONS] <REGION-SET>");
    fprintf(stderr, "Links consecutive regions to produce a non-overlapping set.\n\n"
                    "  * Input formats: BED\n  * Operand: region-set\n  * Region requirements: single-interval\n"
                    "  * Region-set requirements: sorted by chromosome/(strand)/start\n\n");
    return 1;
  }
  _MESSAGES_ = VERBOSE;

  // :686-704: a file or stdin, streamed, its header echoed
  char *REG_FILE = next_arg == argc ? NULL : argv[next_arg];
  GenomicRegionSet RegSet(REG_FILE, BUFFER_SIZE, VERBOSE, false, false);
  RegSet.RunGlobalLink(SORTED_BY_STRAND, LINK_MAX_DIFFERENCE, (char *)LINK_LABEL_FUNC);
  GtxMark("output written");
  GtxFinish(0);
  return 0;
}
