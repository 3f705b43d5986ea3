/* the window selection in one host loop on one core (bench_peakdiff.py: what a tool does today with the scans' vectors on the host):
 * returns the number kept; ordinals and rows as gtx_window_select writes them */
#include <stdint.h>
int64_t select_walk(const uint64_t *const *tested, const uint64_t *const *control, int n_tested, int64_t n, int32_t W, const int32_t *const *kcrit,
                    int64_t *ordinals, int32_t *rows)
{
  const int cols = control ? 2 * n_tested : n_tested;
  int64_t kept = 0;
  for (int64_t i = 0; i < n; i++) {
    int32_t k[4], c[4] = {0, 0, 0, 0};
    int keep = 0;
    for (int f = 0; f < n_tested; f++) {
      const uint64_t v = tested[f][i];
      k[f] = (int32_t)(v < (uint64_t)W ? v : (uint64_t)W);
      if (control) { const uint64_t q = control[f][i]; c[f] = (int32_t)(q < (uint64_t)W ? q : (uint64_t)W); }
      keep |= k[f] >= kcrit[f][c[f]];
    }
    if (!keep) continue;
    ordinals[kept] = i;
    for (int f = 0; f < n_tested; f++) { rows[kept * cols + f] = k[f]; if (control) rows[kept * cols + n_tested + f] = c[f]; }
    kept++;
  }
  return kept;
}
