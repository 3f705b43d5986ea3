// genomic_annotate -- MI355X edition of the `annotate` operation of GenomicTools' genomic_overlaps (reference driver:
// gtools/genomic_overlaps.cpp:185-201 options, :298-305, :310-353 annotate, PrintAnnotations :268-290): for every test region the
// genes it falls in and the upstream regions it falls in, with the offset from the transcription start and, under --distance-flag,
// whether the hit is proximal or distal.  Same command line behind the operation word, same output, same errors.  The upstream
// regions are made on the host (CreateGenomicRegionSetAnnotator, gtools/genomic_intervals.cpp:6218-6297); genes and upstream
// regions then form one reference set on the device, and the pairs of every test region come from its join with the per-pair rule
// applied there (GtxPrintAnnotations: gtx_join_annotate), i.e. HIP kernels through libgtx.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_annotate";
static const long int BUFFER_SIZE = 10000;

int main(int argc, char *argv[])
{
  GtxAcceptSAM(false);                                        // (BED only: SAM stays unsupported, as for the other per-pair tools)
  bool HELP, HELP2, VERBOSE, IS_SORTED, SORTED_BY_STRAND, IGNORE_STRAND, DISTANCE_FLAG, PRINT_HEADER;
  const char *BIN_BITS, *QUERY_OP;
  long int UPSTREAM_MAX_DISTANCE, UPSTREAM_MIN_DISTANCE, PROXIMAL_DIST;
  gtxhost::Options opts;
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  opts.Str("-B", &BIN_BITS, "17,20,23,26", "number of shift-bits for each bin level");
  opts.Flag("-S", &IS_SORTED, "test and reference regions are sorted by chromosome and start position");
  opts.Flag("-s", &SORTED_BY_STRAND, "test and reference regions are also sorted by strand (-S must be set)");
  opts.Flag("-i", &IGNORE_STRAND, "ignore strand while finding overlaps");
  opts.Str("--query-op", &QUERY_OP, "center", "query operation for comparison with reference: {center|overlap}");
  opts.Long("--upstream-max", &UPSTREAM_MAX_DISTANCE, 10000, "maximum allowed upstream region size");
  opts.Long("--upstream-min", &UPSTREAM_MIN_DISTANCE, 10000, "minimum allowed upstream region size (subject to genomic bounds)");
  opts.Flag("--distance-flag", &DISTANCE_FLAG, "add proximal-distal indication");
  opts.Long("--proximal-dist", &PROXIMAL_DIST, 1000, "define proximal distance (in nucleotides)");
  opts.Flag("--print-header", &PRINT_HEADER, "print header");
  int next_arg = opts.Parse(argc, argv, 1);
  if (HELP || HELP2 || argc - next_arg < 1) { opts.Usage(PROGRAM, "[OPTIONS]", "REFERENCE-REGION-FILE <TEST-REGION-FILE>"); return 1; }
  _MESSAGES_ = VERBOSE;

  if (IS_SORTED && SORTED_BY_STRAND && IGNORE_STRAND) {
    fprintf(stderr, "[Error]: the input is sorted by chromosome/strand/start (i.e. -S and -s are set), therefore the overlap algorithm can only report strand-specific results (i.e. -i cannot be set)!\n");
    return 1;
  }

  // :310-327 (the first annotate branch takes every call, -S or not): the test set is streamed, the reference set loaded and
  // checked as its index's constructor does (:5365), then the upstream set made from it
  char *REF_REG_FILE = argv[next_arg];
  char *TEST_REG_FILE = next_arg + 1 == argc ? NULL : argv[next_arg + 1];
  GenomicRegionSet TestRegSet(TEST_REG_FILE, BUFFER_SIZE, VERBOSE, false, true);
  GenomicRegionSet RefRegSet(REF_REG_FILE, BUFFER_SIZE, VERBOSE, true, true);
  for (long int k = 0; k < RefRegSet.n_regions; k++)
    if (!RefRegSet.R[k]->IsCompatibleSortedAndNonoverlapping()) RefRegSet.R[k]->PrintError("index regions should be compatible, sorted and non-overlapping!");
  StringLIntMap *bounds = NULL;
  GenomicRegionSet *UpstreamRefRegSet = NULL;
  if (UPSTREAM_MAX_DISTANCE > 0)
    UpstreamRefRegSet = CreateGenomicRegionSetAnnotator(&RefRegSet, bounds, IGNORE_STRAND, UPSTREAM_MAX_DISTANCE, UPSTREAM_MIN_DISTANCE, (char *)BIN_BITS);
  GtxPrintAnnotations(&TestRegSet, &RefRegSet, UpstreamRefRegSet, QUERY_OP, IGNORE_STRAND, DISTANCE_FLAG, PROXIMAL_DIST, PRINT_HEADER, BIN_BITS);
  GtxMark("output written");
  GtxFinish(0);
  delete UpstreamRefRegSet;
  return 0;
}
