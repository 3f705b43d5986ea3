// annotator_caller -- CreateGenomicRegionSetAnnotator of this package's csrc/genomic_intervals.h called the way the reference's
// `genomic_regions annotator` calls it (gtools/genomic_intervals.cpp:4481-4491, options gtools/genomic_regions.cpp:479-484): the set
// loaded in memory, bin bits "17,20,23,26", the result printed region by region as REG lines ("LABEL\tCHROMOSOME STRAND START STOP").
//   annotator_caller [-g GENOME-REGION-FILE] [-i] [--upstream-max N] [--upstream-min N] REGION-SET
// It exists so that bounds and trimming, which genomic_annotate never uses with bounds, are checked without a GPU.  An input error ends
// the run the way the class layer ends it (message on stderr, exit status 1).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "genomic_intervals.h"

int main(int argc, char **argv)
{
  const char *genome = "";
  bool ignore_strand = false;
  long int upstream_max = 1000000, upstream_min = 10000;
  int a = 1;
  for (; a < argc && argv[a][0] == '-'; a++) {
    if (!strcmp(argv[a], "-i")) ignore_strand = true;
    else if (!strcmp(argv[a], "-g") && a + 1 < argc) genome = argv[++a];
    else if (!strcmp(argv[a], "--upstream-max") && a + 1 < argc) upstream_max = atol(argv[++a]);
    else if (!strcmp(argv[a], "--upstream-min") && a + 1 < argc) upstream_min = atol(argv[++a]);
    else { fprintf(stderr, "unknown option %s\n", argv[a]); return 2; }
  }
  if (argc - a < 1) { fprintf(stderr, "usage: annotator_caller [-g GENOME-REGION-FILE] [-i] [--upstream-max N] [--upstream-min N] REGION-SET\n"); return 2; }
  StringLIntMap *bounds = strlen(genome) > 0 ? ReadBounds((char *)genome) : NULL;
  GenomicRegionSet RegSet(argv[a], 10000, false, true, true);
  if (RegSet.n_regions == 0) return 0;
  char bin_bits[] = "17,20,23,26";
  GenomicRegionSet *up = CreateGenomicRegionSetAnnotator(&RegSet, bounds, ignore_strand, upstream_max, upstream_min, bin_bits);
  for (GenomicRegion *r = up->Get(); r != NULL; r = up->Next()) {
    printf("%s\t", r->LABEL);
    r->I[0]->PrintInterval();
    printf("\n");
  }
  delete up;
  delete bounds;
  return 0;
}
