// windows_caller -- the host loop of GenomicRegionSet::RunSlidingWindows of this package's csrc/genomic_intervals.h, called the way
// the reference's genomic_regions calls it (gtools/genomic_regions.cpp:734): the set streamed, its header echoed.
//   windows_caller STEP SIZE SMALL(0|1) REGION-SET
// It says GTX_TEXT_ON_DEVICE=0 itself, so no device is looked for: every line takes the loop, which is what is checked here without
// a GPU.  An input error ends the run the way the class layer ends it (message on stderr behind the output in front of it, exit
// status 1).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "genomic_intervals.h"

int main(int argc, char **argv)
{
  setenv("GTX_TEXT_ON_DEVICE", "0", 1);
  if (argc != 5) { fprintf(stderr, "usage: windows_caller STEP SIZE SMALL(0|1) REGION-SET\n"); return 2; }
  GenomicRegionSet RegSet(argv[4], 10000, false, false, false);
  RegSet.RunSlidingWindows(atol(argv[1]), atol(argv[2]), atol(argv[3]) != 0);
  fflush(stdout);
  return 0;
}
