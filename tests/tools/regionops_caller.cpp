// regionops_caller -- the host loop of GenomicRegionSet::RunShiftPos / RunModifyPos / RunCenter / RunFix / RunBounds of this package's
// csrc/genomic_intervals.h, called the way the reference's genomic_regions calls them (gtools/genomic_regions.cpp:703-727): the set
// streamed, its header echoed.
//   regionops_caller shift A B | shiftp A B | pos OP K | center | fix | bounds GENOME-REGION-FILE   REGION-SET
// It says GTX_TEXT_ON_DEVICE=0 itself, so no device is looked for: every line takes the loop, which is what is checked here without
// a GPU.  An input error ends the run the way the class layer ends it (message on stderr behind the output in front of it, exit
// status 1).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "genomic_intervals.h"

int main(int argc, char **argv)
{
  setenv("GTX_TEXT_ON_DEVICE", "0", 1);
  const std::string op = argc > 1 ? argv[1] : "";
  const int n_args = op == "shift" || op == "shiftp" || op == "pos" ? 2 : op == "bounds" ? 1 : op == "center" || op == "fix" ? 0 : -1;
  if (n_args < 0 || argc != 3 + n_args) { fprintf(stderr, "usage: regionops_caller shift A B | shiftp A B | pos OP K | center | fix | bounds GENOME-REGION-FILE   REGION-SET\n"); return 2; }
  StringLIntMap *bounds = op == "bounds" ? ReadBounds(argv[2]) : NULL;
  GenomicRegionSet RegSet(argv[2 + n_args], 10000, false, false, false);
  if (op == "shift" || op == "shiftp") RegSet.RunShiftPos(atol(argv[2]), atol(argv[3]), op == "shiftp");
  else if (op == "pos") RegSet.RunModifyPos(argv[2], atol(argv[3]));
  else if (op == "center") RegSet.RunCenter();
  else if (op == "fix") RegSet.RunFix();
  else RegSet.RunBounds(bounds);
  fflush(stdout);
  delete bounds;
  return 0;
}
