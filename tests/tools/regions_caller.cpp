// regions_caller -- a GenomicRegionSet of this package's csrc/genomic_intervals.h opened and walked the way the reference's tools walk
// one (Get / Next), its regions printed one per line:
//   regions_caller [--show-header] [--in-memory] [--refuse] [FILE]        (no FILE: stdin)
//   output: "format = F" first, then per region "LINE\tLABEL\tCHROMOSOME STRAND START STOP" (the strand byte as it stands)
// --show-header opens the set with hide_header = false: the leading '@' or '##' lines of a SAM or GFF file are echoed to stdout in
// front of everything else, as the reference's ProcessFileHeader does.  --refuse calls GtxAcceptSAM(false) first, like the drivers
// that print lines.  It exists so that the class layer's reading of a file -- format detection, header lines, GenomicRegionGFF -- is
// checked without a GPU.  An input error ends the run the way the class layer ends it (message on stderr, exit status 1).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "genomic_intervals.h"

int main(int argc, char **argv)
{
  bool show_header = false, in_memory = false;
  int a = 1;
  for (; a < argc && argv[a][0] == '-'; a++) {
    if (!strcmp(argv[a], "--show-header")) show_header = true;
    else if (!strcmp(argv[a], "--in-memory")) in_memory = true;
    else if (!strcmp(argv[a], "--refuse")) GtxAcceptSAM(false);
    else { fprintf(stderr, "unknown option %s\n", argv[a]); return 2; }
  }
  GenomicRegionSet RegSet(a < argc ? argv[a] : NULL, 10000, false, in_memory, !show_header);
  printf("format = %s\n", RegSet.format.c_str());
  for (GenomicRegion *r = RegSet.Get(); r != NULL; r = RegSet.Next()) {
    GenomicRegionGFF *g = dynamic_cast<GenomicRegionGFF *>(r);
    printf("%ld\t%s\t", r->n_line, r->LABEL);
    r->I[0]->PrintInterval();
    if (g) printf("\t%ld %s %s %s %c %s", g->n_tokens, g->SOURCE, g->FEATURE, g->SCORE, g->FRAME ? g->FRAME : '0', g->COMMENT ? g->COMMENT : "(null)");
    printf("\n");
  }
  return 0;
}
