// genomic_convert -- MI355X edition of the two format conversions of GenomicTools' genomic_regions that open the text pipeline to
// alignments and annotations (reference driver: gtools/genomic_regions.cpp:205-211 and :301-307 operations, :485-490 and :583-585
// options, :686-704 the set with its header hidden, :710 and :722 the calls):
//   bed    every region of a SAM or GFF / GTF set as a BED line (BED12 for a spliced read)
//   reg    every region of a SAM, GFF / GTF or BED set as a line of the toolkit's REG format
// Same command line behind the operation word, same output, same errors.  Single-interval regions are printed on the device
// (GenomicRegionSet::RunConvertToBED / RunConvertToREG: gtx_convert_text / gtx_convert_result), i.e. HIP kernels through libgtx.so.
// genomic_regions keeps refusing the two words; this tool is where they live.
//
// One difference: `bed` on a BED set is refused.  The reference prints such a region through GenomicRegionBED's own members, which
// this build's class does not have.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_convert";
static const long int BUFFER_SIZE = 10000;

static void Usage()
{
  fprintf(stderr, "\nUSAGE: \n  %s OPERATION [OPTIONS] <REGION-SET>\n\nOPERATIONS (MI355X path): \n"
                  "  bed        Converts input regions into BED format.\n"
                  "  reg        Converts to REG format.\n\n", PROGRAM);
}

int main(int argc, char *argv[])
{
  GtxAcceptSAM(true);
  if (argc < 2) { Usage(); return 1; }
  const std::string op = argv[1];
  if (op != "bed" && op != "reg") { fprintf(stderr, "Unknown operation '%s'!\n", op.c_str()); return 1; }

  bool HELP, HELP2, VERBOSE, CONVERT_CHROMOSOME = false, PRINT_COMPACT = false;
  const char *TRACK_TITLE = "", *TRACK_COLOR = "", *TRACK_POSITION = "";
  gtxhost::Options opts;
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  const char *about, *needs;
  if (op == "bed") {                                          // :485-490
    opts.Str("-t", &TRACK_TITLE, "", "title");
    opts.Str("-c", &TRACK_COLOR, "", "color");
    opts.Str("-p", &TRACK_POSITION, "", "browser position");
    opts.Flag("-chr", &CONVERT_CHROMOSOME, "convert chromosome names from ENSEMBL to UCSC");
    about = "Converts input regions into BED format.";
    needs = "  * Input formats: GFF, SAM\n  * Operand: region\n  * Region requirements: chromosome/strand-compatible, sorted, non-overlapping\n"
            "  * Region-set requirements: none\n\n";
  } else {                                                    // :583-585
    opts.Flag("-c", &PRINT_COMPACT, "print in compact starts/ends format");
    about = "Converts to REG format.";
    needs = "  * Input formats: GFF, BED, SAM\n  * Operand: interval\n  * Region requirements: chromosome/strand-compatible if option -c is set\n"
            "  * Region-set requirements: none\n\n";
  }
  const int next_arg = opts.Parse(argc, argv, 2);
  if (HELP || HELP2) {
    opts.Usage(PROGRAM, op.c_str(), "[OPTIONS] <REGION-SET>");
    fprintf(stderr, "%s\n\n%s", about, needs);
    return 1;
  }
  _MESSAGES_ = VERBOSE;

  // :686-704: a file or stdin, streamed, its header hidden (:702)
  char *REG_FILE = next_arg == argc ? NULL : argv[next_arg];
  GenomicRegionSet RegSet(REG_FILE, BUFFER_SIZE, VERBOSE, false, true);
  if (op == "bed" && RegSet.format == "BED") { fprintf(stderr, "Error: the bed operation takes SAM and GFF input: a BED set is not converted into BED!\n"); GtxFinish(1); return 1; }
  if (op == "bed") RegSet.RunConvertToBED((char *)TRACK_TITLE, (char *)TRACK_COLOR, (char *)TRACK_POSITION, CONVERT_CHROMOSOME);
  else RegSet.RunConvertToREG(PRINT_COMPACT);
  GtxMark("output written");
  GtxFinish(0);
  return 0;
}
