// subset_caller -- the reference's `subset` loop (gtools/genomic_overlaps.cpp:794-795) run on the class API of this package's
// csrc/genomic_intervals.h, whose iterators tests/test_class_api.py holds to the checker's: ONE GetOverlap per query, and with -inv
// the loop goes on while there is a query, otherwise until Done().
//   subset_caller [-S] [-s] [-i] [-gaps] [-inv] [-full] REF QUERY
// stdout: "<query line>\t<1 when the reference would print it, else 0>" for every query the loop reads; an input error ends the
// run the way the class layer ends it (message on stderr, exit status 1).  -full: every match is walked (GetOverlap, then
// NextOverlap until NULL) instead of the single call -- what `overlap` does -- to see whether the loop then stops elsewhere.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "genomic_intervals.h"

int main(int argc, char **argv)
{
  bool sorted = false, by_strand = false, ignore_strand = false, gaps = false, inv = false, full = false;
  int a = 1;
  for (; a < argc && argv[a][0] == '-'; a++) {
    if (!strcmp(argv[a], "-S")) sorted = true; else if (!strcmp(argv[a], "-s")) by_strand = true; else if (!strcmp(argv[a], "-i")) ignore_strand = true;
    else if (!strcmp(argv[a], "-gaps")) gaps = true; else if (!strcmp(argv[a], "-inv")) inv = true; else if (!strcmp(argv[a], "-full")) full = true;
    else { fprintf(stderr, "unknown option %s\n", argv[a]); return 2; }
  }
  if (argc - a < 2) { fprintf(stderr, "usage: subset_caller [-S] [-s] [-i] [-gaps] [-inv] [-full] REF QUERY\n"); return 2; }
  GenomicRegionSet RefRegSet(argv[a], 10000, false, true, true);
  GenomicRegionSet TestRegSet(argv[a + 1], 10000, false, false, true);
  GenomicRegionSetOverlaps *overlaps;
  if (sorted) overlaps = new SortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, by_strand);
  else overlaps = new UnsortedGenomicRegionSetOverlaps(&TestRegSet, &RefRegSet, "17,20,23,26");
  for (GenomicRegion *qreg = overlaps->GetQuery(); (inv && (qreg != NULL)) || (overlaps->Done() == false); qreg = overlaps->NextQuery()) {
    GenomicRegion *ireg = overlaps->GetOverlap(gaps, ignore_strand);
    const bool none = ireg == NULL;
    if (full) while (ireg != NULL) ireg = overlaps->NextOverlap(gaps, ignore_strand);
    printf("%ld\t%d\n", qreg->n_line, (none == inv) ? 1 : 0);
    fflush(stdout);
  }
  delete overlaps;
  return 0;
}
