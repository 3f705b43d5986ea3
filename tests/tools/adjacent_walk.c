/* The one-core host walks of packed (class, start, stop) triples that bench_adjacent.py times beside gtx_adjacent_device and
 * gtx_gaps_device: the pair loop of `genomic_regions test` / `gdist` (first unsorted region, inclusions, overlaps, optionally one
 * int64 distance per region) and the gap loop of `genomic_regions inv`.  Measurement only; built by bench_adjacent.py. */
#include <stdint.h>

static int64_t point_of(const int32_t *t, int minus, int op) { return op == 0 ? t[1] : op == 1 ? t[2] : ((op == 2) != (minus != 0)) ? t[1] : t[2]; }

/* info: first_unsorted, n_inclusions, n_overlaps */
void adjacent_walk(const int32_t *tri, const uint8_t *minus, int64_t n, int op1, int op2, int64_t *dist, int64_t *info)
{
  int64_t first = -1, in = 0, ov = 0;
  if (dist && n > 0) dist[0] = INT64_MIN;
  for (int64_t i = 1; i < n; i++) {
    const int32_t *p = tri + 3 * (i - 1), *r = tri + 3 * i;
    if (first < 0 && (r[0] < p[0] || (r[0] == p[0] && r[1] < p[1]))) first = i;
    if (r[0] != p[0]) { if (dist) dist[i] = INT64_MIN; continue; }
    if (r[1] <= p[2]) { if (r[2] <= p[2]) in++; else ov++; }
    if (dist) dist[i] = point_of(r, minus ? minus[i] : 0, op2) - point_of(p, minus ? minus[i - 1] : 0, op1);
  }
  info[0] = first; info[1] = in; info[2] = ov;
}

/* returns the number of gaps written; info: first_bad, bad_kind */
int64_t gaps_walk(const int32_t *tri, int64_t n, const int64_t *bounds, int32_t n_bounds, uint32_t *owner, int32_t *start, int32_t *stop, int64_t *info)
{
  int64_t g = 0, i = 0;
  info[0] = -1; info[1] = 0;
  while (i < n) {
    const int32_t c = tri[3 * i];
    if (c < 0 || c >= n_bounds || bounds[c] < 0) { info[0] = i; info[1] = 2; return g; }
    const int64_t size = bounds[c];
    if (tri[3 * i + 1] > 1) { owner[g] = (uint32_t)i; start[g] = 1; stop[g] = tri[3 * i + 1] - 1; g++; }
    for (i++; i < n && tri[3 * i] == c; i++) {
      if (tri[3 * i + 1] < tri[3 * i - 2]) { info[0] = i; info[1] = 1; return g; }
      if ((int64_t)tri[3 * i + 1] > (int64_t)tri[3 * i - 1] + 1) { owner[g] = (uint32_t)i; start[g] = tri[3 * i - 1] + 1; stop[g] = tri[3 * i + 1] - 1; g++; }
    }
    if ((int64_t)tri[3 * i - 1] + 1 < size) { owner[g] = (uint32_t)(i - 1); start[g] = tri[3 * i - 1] + 1; stop[g] = (int32_t)size; g++; }
  }
  return g;
}
