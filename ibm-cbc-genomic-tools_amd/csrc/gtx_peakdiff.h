// gtx_peakdiff.h -- the binomial rule of `genomic_apps peakdiff` (ScanReadFiles, genomic_apps.cpp:393-403) as tables of critical
// counts, host-only.  The reference keeps a window when gsl_cdf_binomial_Q(k, p, W) <= cutoff for some file, with k the file's clamped
// count and p = max(p_background, min(c / W, 1)) for a control count c (p_background without controls).  The tail does not rise with
// k, so per control count there is one smallest k that passes: the window selection on the device (gtx_window_select) compares
// against that instead of evaluating a tail per window and file.
#pragma once
#include <algorithm>
#include <vector>
#include "gtx_stats.h"

namespace gtxstats {

// kcrit[c] for c in [0, W] (with_control) or for c = 0 alone: the smallest k in [0, W] with BinomialQ(k, p(c), W) <= cutoff, W + 1 when
// there is none.  Found by bisection over k.  The true tail does not rise with k; the computed one changes sides at the mean (a direct
// sum above it, a complement below it), so the answer is then settled by a walk: down while the count below still passes, up while
// the count itself does not.
inline std::vector<int> CriticalCounts(double p_background, long W, double cutoff, bool with_control)
{
  std::vector<int> kcrit((size_t)(with_control ? W + 1 : 1));
  for (size_t c = 0; c < kcrit.size(); c++) {
    const double p = with_control ? std::max(p_background, std::min((double)c / W, 1.0)) : p_background;
    auto passes = [&](long k) { return BinomialQ(k, p, W) <= cutoff; };
    long lo = 0, hi = W + 1;                                         // the answer lies in [lo, hi]
    while (lo < hi) {
      const long mid = lo + (hi - lo) / 2;
      if (passes(mid)) hi = mid; else lo = mid + 1;
    }
    while (lo > 0 && passes(lo - 1)) lo--;
    while (lo <= W && !passes(lo)) lo++;
    kcrit[c] = (int)lo;
  }
  return kcrit;
}

}  // namespace gtxstats
