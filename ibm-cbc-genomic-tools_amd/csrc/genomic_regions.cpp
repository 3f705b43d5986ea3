// genomic_regions -- MI355X edition of seven operations of GenomicTools' genomic_regions, each with the reference's command line
// behind the operation word, the reference's output and errors.
//
//   link     (reference driver: gtools/genomic_regions.cpp:437-451 operation, :469-471 and :546-550 options, :744 the call): a
//            position-sorted region set merged into its covered territory, one "label TAB chromosome strand start stop" line per
//            group -- what `bedtools merge` does.  The group boundaries, the groups' stops and the integer label folds come from the
//            device (GenomicRegionSet::RunGlobalLink: gtx_link)
//   shift, shiftp, pos, center, fix, bounds   (:213-227, :269-275, :293-299, :333-347 operations, :497-499, :579-582, :606-613
//            options, :703-727 the calls): the line-based interval operations in front of a read pipeline -- shift reads by half a
//            fragment, extend them 3', reduce genes to their TSS and widen them, clamp to the chromosome, drop what fell off.  Every
//            BED line printed again with columns 2 and 3 rewritten, or dropped, on the device (GenomicRegionSet::RunShiftPos,
//            RunModifyPos, RunCenter, RunFix, RunBounds: gtx_rewrite_text); header lines are echoed (:702-704)
//
// All through HIP kernels in libgtx.so.  The set is a file or stdin, streamed (:686-704).
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
static const char *OTHER_OPERATIONS[] = {"align", "annotator", "bed", "chrom", "connect", "diff", "dist", "divide", "int", "n",
                                         "reg", "rnd", "search", "select", "shuffle", "sort", "split", "strand", "union", "wig", "win", "x",
                                         "gdist", "gsort", "inv", "test", NULL};

// the operations of this build: word, description (:213-227, :269-275, :293-299, :333-347, :437-451)
struct Operation { const char *word, *text; };
static const Operation OPERATIONS[] = {
  {"bounds", "Trims start/stop positions given the chromosome bounds and removes invalid intervals."},
  {"center", "Prints center interval."},
  {"fix", "Removes invalid intervals, i.e. start<1 or start>stop."},
  {"link", "Links consecutive regions to produce a non-overlapping set."},
  {"pos", "Modifies interval start/stop positions."},
  {"shift", "Shifts interval start/stop positions."},
  {"shiftp", "Shifts interval 5'/3' positions."},
  {NULL, NULL}};

// shift, shiftp, pos, center, fix, bounds: options, help, the set with its header echoed, the call
static int interval_operation(const Operation &o, int argc, char *argv[])
{
  const std::string op = o.word;
  bool HELP, HELP2, VERBOSE;
  long SHIFT_A = 0, SHIFT_B = 0, POSITION_SHIFT = 0;
  const char *GENOME_REG_FILE = NULL, *POSITION_OP = "1";
  gtxhost::Options opts;
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  if (op == "bounds") opts.Str("-g", &GENOME_REG_FILE, "", "genome region-set file");                      // :497-499
  else if (op == "pos") {                                                                                 // :579-582
    opts.Str("-op", &POSITION_OP, "1", "position operation (1=start, 2=stop, 5p=5'-end, 3p=3'-end, c=center)");
    opts.Long("-c", &POSITION_SHIFT, 0, "position shift");
  } else if (op == "shift") {                                                                             // :606-609
    opts.Long("-start", &SHIFT_A, 0, "shift distance for start position");
    opts.Long("-stop", &SHIFT_B, 0, "shift distance for stop position");
  } else if (op == "shiftp") {                                                                            // :610-613
    opts.Long("-5p", &SHIFT_A, 0, "shift distance for 5' end");
    opts.Long("-3p", &SHIFT_B, 0, "shift distance for 3' end");
  }
  const int next_arg = opts.Parse(argc, argv, 2);
  if (HELP || HELP2) {
    opts.Usage(PROGRAM, o.word, "[OPTIONS] <REGION-SET>");
    fprintf(stderr, "%s\n\n  * Input formats: BED\n  * Operand: interval\n  * Region requirements: none\n"
                    "  * Region-set requirements: none\n\n", o.text);
    return 1;
  }
  _MESSAGES_ = VERBOSE;
  // :693: the bounds before the set is opened; `bounds` without -g ends in ReadBounds' error
  StringLIntMap *bounds = GENOME_REG_FILE == NULL ? NULL : ReadBounds((char *)GENOME_REG_FILE, VERBOSE);
  char *REG_FILE = next_arg == argc ? NULL : argv[next_arg];
  GenomicRegionSet RegSet(REG_FILE, BUFFER_SIZE, VERBOSE, false, false);
  if (op == "bounds") RegSet.RunBounds(bounds);
  else if (op == "center") RegSet.RunCenter();
  else if (op == "fix") RegSet.RunFix();
  else if (op == "pos") RegSet.RunModifyPos(POSITION_OP, POSITION_SHIFT);
  else RegSet.RunShiftPos(SHIFT_A, SHIFT_B, op == "shiftp");
  GtxMark("output written");
  GtxFinish(0);
  return 0;
}

int main(int argc, char *argv[])
{
  GtxAcceptSAM(false);                                        // (the groups print the head's label: SAM stays unsupported, as for the tools that print lines)
  if (argc < 2) {
    fprintf(stderr, "\nUSAGE: \n  %s OPERATION [OPTIONS] <REGION-SET>\n\nOPERATIONS (MI355X path): \n", PROGRAM);
    for (const Operation *o = OPERATIONS; o->word; o++) fprintf(stderr, "  %-10s %s\n", o->word, o->text);
    fprintf(stderr, "\n");
    return 1;
  }
  const std::string op = argv[1];
  for (const char **o = OTHER_OPERATIONS; *o; o++)
    if (op == *o) { fprintf(stderr, "Operation '%s' is outside the MI355X path of this build!\n", *o); return 1; }
  for (const Operation *o = OPERATIONS; o->word; o++)
    if (op == o->word && op != "link") return interval_operation(*o, argc, argv);
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
