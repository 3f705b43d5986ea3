/* The one-core host walk of packed (class, start, stop) triples that bench_link.py times beside gtx_link_device: the loop of
 * `genomic_regions link` (group while START - new_stop <= d within a class) with an optional int64 sum per group.  Measurement
 * only; built by bench_link.py. */
#include <stdint.h>

int64_t link_walk(const int32_t *tri, const int64_t *vals, int64_t n, int64_t d, uint32_t *head, uint32_t *count, int32_t *stop, int64_t *sum,
                  int64_t *first_unsorted)
{
  int64_t g = 0, i = 0;
  *first_unsorted = -1;
  while (i < n) {
    const int64_t h = i;
    const int32_t c = tri[3 * i];
    int32_t new_stop = tri[3 * i + 2];
    int64_t acc = vals ? vals[i] : 0;
    for (i++; i < n; i++) {
      const int32_t ci = tri[3 * i], si = tri[3 * i + 1];
      if (ci < tri[3 * i - 3] || (ci == tri[3 * i - 3] && si < tri[3 * i - 2])) { *first_unsorted = i; return g; }
      if (ci != c || (int64_t)si - (int64_t)new_stop > d) break;
      if (tri[3 * i + 2] > new_stop) new_stop = tri[3 * i + 2];
      if (vals) acc += vals[i];
    }
    head[g] = (uint32_t)h; count[g] = (uint32_t)(i - h); stop[g] = new_stop;
    if (vals) sum[g] = acc;
    g++;
  }
  return g;
}
