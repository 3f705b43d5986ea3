// genomic_overlaps -- MI355X edition of the `count`, `rpkm`, `coverage`, `density`, `offset`, `overlap`
// and `intersect` operations of GenomicTools' genomic_overlaps (reference driver: gtools/genomic_overlaps.cpp:
// 73-261 options, :298-305, :408-431 count, :438-459 coverage, :466-490 density, :545-670 offset,
// :676-701 intersect, :706-741 overlap, :746-775 rpkm).  Same command line, same output, same errors; the
// reductions are GenomicRegionSetOverlaps::CountIndexOverlaps / CalcIndexCoverage of this package, the pairs
// of overlap / intersect come from the device join (GtxPrintPairs) and those of offset with their offsets
// (GtxPrintOffsets), i.e. HIP kernels through libgtx.so.  annotate, bin, dist and subset are outside this path.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_overlaps";
static const long int BUFFER_SIZE = 10000;

int main(int argc, char *argv[])
{
  if (argc < 2) {
    fprintf(stderr, "\nUSAGE: \n  %s OPERATION [OPTIONS] REFERENCE-REGION-FILE <TEST-REGION-FILE>\n\nOPERATIONS (MI355X path): \n"
                    "  count      Counts the number of overlapping test regions per reference region.\n"
                    "  coverage   Calculates the depth coverage (total number of overlapping nucleotides) per reference region.\n"
                    "  density    Computes the density (coverage divided by the size of the reference region) per reference region.\n"
                    "  intersect  Prints the test regions clipped to each overlapping reference region.\n"
                    "  offset     Computes the distances of test regions from their overlapping reference regions.\n"
                    "  overlap    Prints the test regions once per overlapping reference region.\n"
                    "  rpkm       Computing reference region RPKM values.\n\n", PROGRAM);
    return 1;
  }
  std::string op = argv[1];
  if (op[0] == '-') op = op.substr(1);                        // compatibility with the old "-count" spelling
  static const char *others[] = {"annotate", "bin", "dist", "subset"};
  for (const char *o : others) if (op == o) { fprintf(stderr, "Operation '%s' is outside the MI355X counting path of this build (count, coverage, density, rpkm)!\n", o); return 1; }
  if (op != "count" && op != "rpkm" && op != "coverage" && op != "density" && op != "overlap" && op != "intersect" && op != "offset") { fprintf(stderr, "Unknown operation '%s'!\n", op.c_str()); return 1; }
  const bool per_pair = op == "overlap" || op == "intersect";
  if (per_pair || op == "offset") GtxAcceptSAM(false);        // (they print query lines in their own format: SAM stays unsupported there)

  bool HELP, HELP2, VERBOSE, IS_SORTED, SORTED_BY_STRAND, IGNORE_STRAND, MATCH_GAPS;
  const char *BIN_BITS; long MAX_LABEL_VALUE; unsigned long MIN_COUNT = 0; double MIN_RPKM, MIN_DENSITY = 0.0;
  gtxhost::Options opts;
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  opts.Str("-B", &BIN_BITS, "17,20,23,26", "number of shift-bits for each bin level (count / coverage: accepted, unused; overlap / intersect / offset: the order of the pairs)");
  opts.Flag("-S", &IS_SORTED, "test and reference regions are sorted by chromosome and start position");
  opts.Flag("-s", &SORTED_BY_STRAND, "test and reference regions are also sorted by strand (-S must be set)");
  opts.Flag("-i", &IGNORE_STRAND, "ignore strand while finding overlaps");
  bool MERGE_LABELS = false;
  MATCH_GAPS = false; MAX_LABEL_VALUE = 1;
  if (op != "intersect") opts.Flag("-gaps", &MATCH_GAPS, "matching gaps between intervals are considered overlaps");
  if (per_pair) opts.Flag("-label", &MERGE_LABELS, "print test and reference labels as test:reference");
  bool SKIP_REF_GAPS = false, FRACTION = false, CENTER = false; const char *OFFSET_OP = "5p";
  if (op == "offset") {                                       // :229-236
    opts.Flag("--skip-ref-gaps", &SKIP_REF_GAPS, "ignore gaps in reference regions when computing offsets");
    opts.Flag("-label", &MERGE_LABELS, "print test region labels");
    opts.Str("-op", &OFFSET_OP, "5p", "reference point (1=start, 2=stop, 5p=5'-end, 3p=3'-end)");
    opts.Flag("-a", &FRACTION, "print distances as a fraction of total size");
    opts.Flag("-c", &CENTER, "print center of interval only");
  }
  if (!per_pair && op != "offset") opts.Long("--max-label-value", &MAX_LABEL_VALUE, 1, "maximum region label value to be used");
  if (op == "count") opts.ULong("-min", &MIN_COUNT, 0, "minimum count");
  else if (op == "coverage") opts.ULong("-min", &MIN_COUNT, 0, "minimum coverage");
  else if (op == "density") opts.Double("-min", &MIN_DENSITY, 0.0, "minimum density");
  else if (op == "rpkm") opts.Double("-min", &MIN_RPKM, 0.0, "minimum RPKM");
  long NGPU = 0; if (!per_pair && op != "offset") opts.Long("--ngpu", &NGPU, 0, "MI355X: number of GPUs the reduction is spread over, by chromosome, RCCL reduce of the result (default: GTX_NGPU or 1)");
  int next_arg = opts.Parse(argc, argv, 2);
  if (NGPU > 0) GtxSetDevices((int)NGPU);
  if (HELP || HELP2 || argc - next_arg < 1) { opts.Usage(PROGRAM, op.c_str(), "[OPTIONS] REFERENCE-REGION-FILE <TEST-REGION-FILE>"); return 1; }
  _MESSAGES_ = VERBOSE;

  if (IS_SORTED && SORTED_BY_STRAND && IGNORE_STRAND) {
    fprintf(stderr, "[Error]: the input is sorted by chromosome/strand/start (i.e. -S and -s are set), therefore the overlap algorithm can only report strand-specific results (i.e. -i cannot be set)!\n");
    return 1;
  }

  char *REF_REG_FILE = argv[next_arg];
  char *TEST_REG_FILE = next_arg + 1 == argc ? NULL : argv[next_arg + 1];
  if (op == "offset") {                                       // :545-670: both sets without their headers
    if (IS_SORTED && SKIP_REF_GAPS) {
      fprintf(stderr, "Error: option --subtract-gaps is not implemented for the -S option. Simply drop the -S and re-run!\n");
      return 1;
    }
    // without -S the reference set is the index (:600-604); under -S the merge's queries are the reference file (:551-555), and
    // the test set, its index, is loaded in memory here
    GenomicRegionSet RefRegSet(REF_REG_FILE, BUFFER_SIZE, VERBOSE, !IS_SORTED, true);
    GenomicRegionSet TestRegSet(TEST_REG_FILE, BUFFER_SIZE, VERBOSE, IS_SORTED, true);
    GenomicRegionSetOverlaps *overlaps;
    if (IS_SORTED) overlaps = new SortedGenomicRegionSetOverlaps(&RefRegSet, &TestRegSet, SORTED_BY_STRAND);
    else overlaps = new UnsortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, BIN_BITS);
    GtxPrintOffsets(overlaps, OFFSET_OP, SKIP_REF_GAPS, FRACTION, CENTER, MERGE_LABELS, MATCH_GAPS, IGNORE_STRAND, BIN_BITS);
    GtxMark("output written");
    GtxFinish(0);
    delete overlaps;
    return 0;
  }
  if (per_pair) {                                             // :676-741: the test set is streamed with its header echoed
    GenomicRegionSet RefRegSet(REF_REG_FILE, BUFFER_SIZE, VERBOSE, true, true);
    GenomicRegionSet TestRegSet(TEST_REG_FILE, BUFFER_SIZE, VERBOSE, false, false);
    GenomicRegionSetOverlaps *overlaps;
    if (IS_SORTED) overlaps = new SortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, SORTED_BY_STRAND);
    else overlaps = new UnsortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, BIN_BITS);
    GtxPrintPairs(overlaps, op == "intersect", MATCH_GAPS, IGNORE_STRAND, MERGE_LABELS, BIN_BITS);
    GtxMark("output written");
    GtxFinish(0);
    delete overlaps;
    return 0;
  }
  GenomicRegionSet RefRegSet(REF_REG_FILE, BUFFER_SIZE, VERBOSE, true, true);
  GenomicRegionSet TestRegSet(TEST_REG_FILE, BUFFER_SIZE, VERBOSE, false, true);

  GenomicRegionSetOverlaps *overlaps;
  if (IS_SORTED) overlaps = new SortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, SORTED_BY_STRAND);
  else overlaps = new UnsortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, BIN_BITS);
  unsigned long int *hits = (op == "coverage" || op == "density") ? overlaps->CalcIndexCoverage(MATCH_GAPS, IGNORE_STRAND, MAX_LABEL_VALUE)
                                                                  : overlaps->CountIndexOverlaps(MATCH_GAPS, IGNORE_STRAND, MAX_LABEL_VALUE);

  if (op == "density") {
    for (long int k = 0; k < RefRegSet.n_regions; k++) {
      long int size = (long int)RefRegSet.R[k]->GetSize(!MATCH_GAPS);
      volatile double density = (double)hits[k] / size;
      if (density >= MIN_DENSITY) printf("%s\t%.4e\n", RefRegSet.R[k]->LABEL, density);
    }
  } else if (op == "count" || op == "coverage") {
    for (long int k = 0; k < RefRegSet.n_regions; k++)
      if (hits[k] >= MIN_COUNT) printf("%s\t%lu\n", RefRegSet.R[k]->LABEL, hits[k]);
  } else {
    unsigned long int nreads = 0;
    for (long int k = 0; k < RefRegSet.n_regions; k++) nreads += hits[k];
    if (VERBOSE) fprintf(stderr, "* %lu reads overlap reference regions.\n", nreads);
    volatile double mreads = (double)nreads / 1000000;
    volatile double zero = 0.0;
    for (long int k = 0; k < RefRegSet.n_regions; k++) {
      long int eff_len = (long int)RefRegSet.R[k]->GetSize(!MATCH_GAPS);
      double rpkm = eff_len <= 0 ? zero / zero : (double)1000 * hits[k] / eff_len / mreads;   // the reference's -min is parsed but never applied
      printf("%s\t%.4e\n", RefRegSet.R[k]->LABEL, rpkm);
    }
  }
  GtxMark("output written");
  GtxFinish(0);
  delete[] hits;
  delete overlaps;
  return 0;
}
