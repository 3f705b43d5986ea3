// gtx_api_join.hip -- the C ABI's entry points over the overlap join: gtx_join*, per-query hits, pair offsets, the annotate pass and
// signal bins.  Host code only (the kernels: gtx_join.hip, gtx_query.hip, gtx_offset.hip, gtx_annotate.hip, gtx_signal.hip); the
// context and the helpers shared with the other families are in gtx_ctx.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <functional>
#include <string>
#include <vector>
#include "gtx.h"
#include "gtx_pairs.h"
#include "gtx_join.h"
#include "gtx_query.h"
#include "gtx_offset.h"
#include "gtx_annotate.h"
#include "gtx_signal.h"
#include "gtx_ctx.h"

// ---------------------------------------------------------------------------------------------
// the overlap join (gtx_join.hip)
// ---------------------------------------------------------------------------------------------

// the envelope index over all regions, and whether a query's pairs come out of the walk already in key order: the emit pass
// writes them by ascending index position, so that holds when (key, ordinal) ascends along the index inside every class --
// ordinal keys on a position-sorted set (the sorted merge's) are the common case
int join_prepare(gtx_ctx *c)
{
  if (!c->rx.pairAll.built) { c->rx.joinMono = -1; int rc = build_pair_index(c, &c->rx.pairAll, [](int64_t) { return true; }); if (rc) return rc; }
  if (c->rx.joinMono >= 0) return GTX_OK;
  const int n = c->rx.pairAll.n, nc = c->nClasses;
  std::vector<int32_t> seg(nc + 1), id(std::max(n, 1));
  HIPCHK(c, hipMemcpy(seg.data(), c->rx.pairAll.ix.seg, sizeof(int32_t) * (nc + 1), hipMemcpyDeviceToHost));
  if (n) HIPCHK(c, hipMemcpy(id.data(), c->rx.pairAll.ix.id, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  const bool keyed = !c->rx.h_joinKey.empty();
  bool mono = true;
  for (int cl = 0; cl < nc && mono; cl++)
    for (int i = seg[cl] + 1; i < seg[cl + 1] && mono; i++) {
      const int32_t a = id[i - 1], b = id[i];
      const long long ka = keyed ? c->rx.h_joinKey[a] : a, kb = keyed ? c->rx.h_joinKey[b] : b;
      mono = ka < kb || (ka == kb && a < b);
    }
  c->rx.joinMono = mono ? 1 : 0;
  return GTX_OK;
}

int join_mode(gtx_ctx *c, uint32_t flags)
{
  return ((flags & GTX_ZERO_LENGTH_OK) ? gtx::JOIN_ZERO_OK : 0) | (c->mergeRefs ? gtx::JOIN_MERGE : 0) |
         ((flags & GTX_CHECK_SORTED) ? gtx::JOIN_CHECK : 0) | ((flags & GTX_JOIN_GAPS) ? gtx::JOIN_GAPS : 0);
}

// count + scan of the n queries into d_off (n + 1 offsets from 0), *total = d_off[n]; info of the count pass in *hi
static int join_count(gtx_ctx *c, const gtx::JoinQueries &q, int mode, long long *d_off, int64_t *total, gtx::JoinInfo *hi)
{
  HIPCHK(c, hipSetDevice(c->device));
  int rc = join_prepare(c); if (rc) return rc;
  if (!c->join.info) HIPCHK(c, c->join.info.alloc(1));
  if (!c->join.cut) HIPCHK(c, c->join.cut.alloc(2));
  HIPCHK(c, c->join.part.grow((size_t)gtx::join_scan_partials(q.n + 1)));
  const gtx::JoinInfo init = {0, 0, INT64_MAX, INT64_MAX, 0};
  HIPCHK(c, hipMemcpyAsync(c->join.info.get(), &init, sizeof init, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gtx::launch_join_count(q, c->rx.pairAll.ix, ref_blocks(c), mode, d_off, c->join.info.get(), c->stream));
  HIPCHK(c, hipMemsetAsync(d_off + q.n, 0, sizeof(long long), c->stream));
  HIPCHK(c, gtx::launch_join_scan(d_off, q.n + 1, c->join.part.get(), c->stream));
  long long t = 0;
  HIPCHK(c, hipMemcpyAsync(&t, d_off + q.n, sizeof t, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hi, c->join.info.get(), sizeof *hi, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *total = t;
  return GTX_OK;
}

// the pairs of queries [q0, q1) into d_pairs (their offsets relative to d_off[q0]), sorted by key; scratch: a buffer as long
static int join_emit(gtx_ctx *c, const gtx::JoinQueries &q, int mode, const long long *d_off, int64_t q0, int64_t q1, int *d_pairs, int *d_scratch)
{
  HIPCHK(c, gtx::launch_join_emit(q, q0, q1, c->rx.pairAll.ix, ref_blocks(c), mode, d_off, d_pairs, c->join.info.get(), c->stream));
  if (!c->rx.joinMono) {
    HIPCHK(c, c->join.big.grow((size_t)(q1 - q0 + 1)));
    HIPCHK(c, gtx::launch_join_sort(d_off, q0, q1, c->rx.joinKey.get(), d_pairs, d_scratch, c->join.big.get(), c->stream));
  }
  long long mismatch = 0;
  HIPCHK(c, hipMemcpyAsync(&mismatch, &c->join.info.get()->mismatch, sizeof mismatch, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (mismatch) return fail(c, GTX_E_HIP, "gtx_join: the emit pass found another number of pairs than the count pass");
  return GTX_OK;
}

// the longest run of queries from q0 whose pairs fit `cap`
static int join_cut(gtx_ctx *c, const long long *d_off, int64_t q0, int64_t n, int64_t cap, int64_t *q1)
{
  HIPCHK(c, gtx::launch_join_cut(d_off, q0, n, cap, c->join.cut.get(), c->stream));
  long long v = 0;
  HIPCHK(c, hipMemcpyAsync(&v, c->join.cut.get(), sizeof v, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *q1 = v;
  return GTX_OK;
}

static void join_info_merge(gtx_count_info *info, const gtx::JoinInfo &h, int64_t base)
{
  info->n_no_class += h.noClass;
  info->n_degenerate += h.degenerate;
  if (h.firstDegenerate != INT64_MAX && info->first_degenerate < 0) info->first_degenerate = h.firstDegenerate + base;
  if (h.firstUnsorted != INT64_MAX && info->first_unsorted < 0) info->first_unsorted = h.firstUnsorted + base;
}

extern "C" {

int gtx_set_ref_order(gtx_ctx *c, const int64_t *key)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_set_ref_order: gtx_set_refs has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rx.joinKey.reset(); c->rx.h_joinKey.clear(); c->rx.joinMono = -1;
  if (!key || c->nRefs == 0) return GTX_OK;
  c->rx.h_joinKey.assign(key, key + c->nRefs);
  HIPCHK(c, upload(c->rx.joinKey, (const long long *)key, (size_t)c->nRefs));
  return GTX_OK;
}

int gtx_set_join_buffer(gtx_ctx *c, int64_t max_pairs)
{
  if (!c) return GTX_E_ARG;
  if (max_pairs < 1) return fail(c, GTX_E_ARG, "gtx_set_join_buffer: at least one pair");
  c->join.buffer = max_pairs;
  return GTX_OK;
}

int gtx_join_device(gtx_ctx *c, const void *d_reads, int64_t n, uint32_t flags, void *d_offsets, void *d_pairs, int64_t cap,
                    int64_t *n_pairs_out, int64_t *n_done_out, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_join_device: gtx_set_refs has not been called");
  if (n < 0 || (n > 0 && !d_reads) || !d_offsets || cap < 0 || (cap > 0 && !d_pairs)) return fail(c, GTX_E_ARG, "gtx_join_device: bad argument");
  const int mode = join_mode(c, flags);
  const gtx::JoinQueries q{(const int *)d_reads, nullptr, nullptr, n};
  long long *off = (long long *)d_offsets;
  int64_t total = 0; gtx::JoinInfo hi;
  int rc = join_count(c, q, mode, off, &total, &hi); if (rc) return rc;
  int64_t q1 = n;
  if (total > cap) { rc = join_cut(c, off, 0, n, cap, &q1); if (rc) return rc; }
  if (q1 > 0) {
    int64_t len = 0;
    if (q1 < n) HIPCHK(c, hipMemcpy(&len, off + q1, sizeof len, hipMemcpyDeviceToHost)); else len = total;
    if (!c->rx.joinMono) { HIPCHK(c, c->join.scratch.grow((size_t)len)); }
    rc = join_emit(c, q, mode, off, 0, q1, (int *)d_pairs, c->join.scratch.get()); if (rc) return rc;
  }
  if (n_pairs_out) *n_pairs_out = total;
  if (n_done_out) *n_done_out = q1;
  if (info) { memset(info, 0, sizeof *info); info->first_unsorted = -1; info->first_degenerate = -1; join_info_merge(info, hi, 0); }
  return GTX_OK;
}

} // extern "C"

// n host queries as gtx_join takes them: triples, and interval lists (first / blocks) or none
static bool queries_ok(const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t n)
{
  return !(n < 0 || (n > 0 && !reads) || (first && (first[0] != 0 || (first[n] > 0 && !blocks))));
}

// queries [b0, b1) into d_joinReads and q pointed at them; with_blocks: their intervals too (when given) into d_joinQBlk /
// d_joinQIv, checked.  qb / iv hold the host copies until the stream has passed the copies
static int stage_queries(gtx_ctx *c, const std::string &w, const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t b0,
                         int64_t b1, bool with_blocks, std::vector<int2> &qb, std::vector<int2> &iv, gtx::JoinQueries &q)
{
  const int64_t m = b1 - b0;
  HIPCHK(c, c->join.reads.grow((size_t)(3 * m)));
  HIPCHK(c, hipMemcpyAsync(c->join.reads.get(), reads + 3 * b0, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, c->stream));
  q = gtx::JoinQueries{c->join.reads.get(), nullptr, nullptr, m};
  if (!first || !with_blocks) return GTX_OK;
  qb.resize((size_t)m);
  const int64_t i0 = first[b0];
  if (first[b1] - i0 >= INT32_MAX) return fail(c, GTX_E_ARG, (w + ": too many intervals in one batch").c_str());
  for (int64_t i = b0; i < b1; i++) {
    const int64_t cnt = first[i + 1] - first[i];
    if (cnt < 1) return fail(c, GTX_E_ARG, (w + ": every query has at least one interval").c_str());
    const int32_t *b = blocks + 2 * first[i];
    if (b[0] != reads[3 * i + 1] || b[2 * cnt - 1] != reads[3 * i + 2]) return fail(c, GTX_E_ARG, (w + ": a query's triple must be its envelope").c_str());
    if (!blocks_monotone(b, cnt)) return fail(c, GTX_E_RANGE, (w + ": the intervals of a query must be sorted (starts and stops non-decreasing)").c_str());
    qb[i - b0] = make_int2((int)(first[i] - i0), (int)cnt);
  }
  iv.resize((size_t)std::max<int64_t>(first[b1] - i0, 1));
  for (int64_t j = i0; j < first[b1]; j++) iv[j - i0] = make_int2(blocks[2 * j], blocks[2 * j + 1]);
  HIPCHK(c, c->join.qBlk.grow(qb.size()));
  HIPCHK(c, c->join.qIv.grow(iv.size()));
  HIPCHK(c, hipMemcpyAsync(c->join.qBlk.get(), qb.data(), sizeof(int2) * qb.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->join.qIv.get(), iv.data(), sizeof(int2) * iv.size(), hipMemcpyHostToDevice, c->stream));
  q.blk = c->join.qBlk.get(); q.iv = c->join.qIv.get();
  return GTX_OK;
}

// the body of gtx_join / gtx_join_offsets: the queries in batches of batchReads, the pairs of each batch in chunks of at most
// joinBuffer pairs.  on_chunk(q, b0, q0, q1, p0, len) runs when the pairs of the batch's queries [q0, q1) are in d_joinPairs (their
// offsets relative to d_joinOff[q0]; p0: the position of the first among all pairs).  all_blocks: the queries' intervals go to
// the device under GTX_JOIN_GAPS too.
typedef std::function<int(const gtx::JoinQueries &, int64_t, int64_t, int64_t, int64_t, int64_t)> JoinChunk;
static int join_batches(gtx_ctx *c, const char *who, const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t n, uint32_t flags,
                        bool all_blocks, int64_t *offsets_out, int64_t cap, gtx_count_info *info, const JoinChunk &on_chunk)
{
  const std::string w(who);
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, (w + ": gtx_set_refs has not been called").c_str());
  if (!offsets_out || cap < 0 || !queries_ok(reads, first, blocks, n)) return fail(c, GTX_E_ARG, (w + ": bad argument").c_str());
  HIPCHK(c, hipSetDevice(c->device));
  const int mode = join_mode(c, flags);
  gtx_count_info acc; memset(&acc, 0, sizeof acc); acc.first_unsorted = -1; acc.first_degenerate = -1;
  int64_t base = 0;                                            // pairs before the batch
  offsets_out[0] = 0;
  const int64_t per = std::max<int64_t>(1, c->batchReads);
  for (int64_t b0 = 0; b0 < n; b0 += per) {
    const int64_t b1 = std::min(n, b0 + per), m = b1 - b0;
    gtx::JoinQueries q{};
    std::vector<int2> qb, iv;
    int rc = stage_queries(c, w, reads, first, blocks, b0, b1, all_blocks || !(mode & gtx::JOIN_GAPS), qb, iv, q); if (rc) return rc;
    HIPCHK(c, c->join.off.grow((size_t)(m + 1)));
    int64_t total = 0; gtx::JoinInfo hi;
    rc = join_count(c, q, mode, c->join.off.get(), &total, &hi); if (rc) return rc;      // (synchronises: qb / iv may go)
    if ((flags & GTX_CHECK_SORTED) && b0 > 0 && acc.first_unsorted < 0) {           // the seam between two batches comes before the batch's own
      const int32_t *p = reads + 3 * (b0 - 1), *r = reads + 3 * b0;
      if (r[0] < p[0] || (r[0] == p[0] && r[1] < p[1])) acc.first_unsorted = b0;
    }
    join_info_merge(&acc, hi, b0);
    HIPCHK(c, hipMemcpy(offsets_out + b0, c->join.off.get(), sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost));
    for (int64_t i = b0; i <= b1; i++) offsets_out[i] += base;
    // pairs chunk by chunk: the longest run of queries that fits the device buffer, or one query alone in a buffer of its size
    const int64_t chunk = std::min<int64_t>(c->join.buffer, std::max<int64_t>(total, 1));
    for (int64_t q0 = 0; q0 < m && offsets_out[b0 + q0] < cap;) {
      int64_t q1 = m;
      if (offsets_out[b1] - offsets_out[b0 + q0] > chunk) { rc = join_cut(c, c->join.off.get(), q0, m, chunk, &q1); if (rc) return rc; }
      if (q1 == q0) q1 = q0 + 1;
      const int64_t p0 = offsets_out[b0 + q0], len = offsets_out[b0 + q1] - p0;
      if (len > 0) {
        HIPCHK(c, c->join.pairs.grow((size_t)len));
        if (!c->rx.joinMono) { HIPCHK(c, c->join.scratch.grow((size_t)len)); }
        rc = join_emit(c, q, mode, c->join.off.get(), q0, q1, c->join.pairs.get(), c->join.scratch.get()); if (rc) return rc;
        rc = on_chunk(q, b0, q0, q1, p0, len); if (rc) return rc;
      }
      q0 = q1;
    }
    base = offsets_out[b1];
  }
  if (info) *info = acc;
  return GTX_OK;
}

extern "C" {

int gtx_join(gtx_ctx *c, const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t n, uint32_t flags,
             int64_t *offsets_out, int32_t *pairs_out, int64_t cap, gtx_count_info *info)
{
  if (c && c->nRefs >= 0 && cap > 0 && !pairs_out) return fail(c, GTX_E_ARG, "gtx_join: bad argument");
  return join_batches(c, "gtx_join", reads, first, blocks, n, flags, false, offsets_out, cap, info,
                      [&](const gtx::JoinQueries &, int64_t, int64_t, int64_t, int64_t p0, int64_t len) {
                        const int64_t keep = std::min(len, cap - p0);
                        HIPCHK(c, hipMemcpy(pairs_out + p0, c->join.pairs.get(), sizeof(int32_t) * keep, hipMemcpyDeviceToHost));
                        return GTX_OK;
                      });
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// per-query hits (gtx_query.hip)
// ---------------------------------------------------------------------------------------------

// d_hits[i] = the pairs of query i, *hi = what the pass observed: the join's count walk, its counts narrowed to 32 bits.  Returns
// with the work complete.
static int hits_pass(gtx_ctx *c, const gtx::JoinQueries &q, int mode, unsigned *d_hits, gtx::JoinInfo *hi)
{
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->join.info) HIPCHK(c, c->join.info.alloc(1));
  const gtx::JoinInfo init = {0, 0, INT64_MAX, INT64_MAX, 0};
  *hi = init;
  if (q.n == 0) return GTX_OK;
  HIPCHK(c, hipMemcpyAsync(c->join.info.get(), &init, sizeof init, hipMemcpyHostToDevice, c->stream));
  int rc = join_prepare(c); if (rc) return rc;
  HIPCHK(c, c->join.off.grow((size_t)q.n));
  HIPCHK(c, gtx::launch_join_count(q, c->rx.pairAll.ix, ref_blocks(c), mode, c->join.off.get(), c->join.info.get(), c->stream));
  HIPCHK(c, gtx::launch_query_narrow(c->join.off.get(), q.n, d_hits, c->stream));
  HIPCHK(c, hipMemcpyAsync(hi, c->join.info.get(), sizeof *hi, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTX_OK;
}

extern "C" {

int gtx_query_hits_device(gtx_ctx *c, const void *d_reads, int64_t n, uint32_t flags, void *d_hits, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_query_hits_device: gtx_set_refs has not been called");
  if (n < 0 || (n > 0 && (!d_reads || !d_hits))) return fail(c, GTX_E_ARG, "gtx_query_hits_device: bad argument");
  const int mode = join_mode(c, flags);
  const gtx::JoinQueries q{(const int *)d_reads, nullptr, nullptr, n};
  gtx::JoinInfo hi;
  int rc = hits_pass(c, q, mode, (unsigned *)d_hits, &hi); if (rc) return rc;
  if (info) { memset(info, 0, sizeof *info); info->first_unsorted = -1; info->first_degenerate = -1; join_info_merge(info, hi, 0); }
  return GTX_OK;
}

int gtx_query_hits(gtx_ctx *c, const int32_t *reads, const int64_t *first, const int32_t *blocks, int64_t n, uint32_t flags,
                   uint32_t *hits_out, gtx_count_info *info)
{
  const std::string w("gtx_query_hits");
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_query_hits: gtx_set_refs has not been called");
  if ((n > 0 && !hits_out) || !queries_ok(reads, first, blocks, n)) return fail(c, GTX_E_ARG, "gtx_query_hits: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  const int mode = join_mode(c, flags);
  const bool with_blocks = first && !(mode & gtx::JOIN_GAPS);   // (under -gaps the envelopes alone decide)
  gtx_count_info acc; memset(&acc, 0, sizeof acc); acc.first_unsorted = -1; acc.first_degenerate = -1;
  const int64_t per = std::max<int64_t>(1, c->batchReads);
  for (int64_t b0 = 0; b0 < n; b0 += per) {
    const int64_t b1 = std::min(n, b0 + per), m = b1 - b0;
    gtx::JoinQueries q{};
    std::vector<int2> qb, iv;
    int rc = stage_queries(c, w, reads, first, blocks, b0, b1, with_blocks, qb, iv, q); if (rc) return rc;
    HIPCHK(c, c->join.hitsOut.grow((size_t)m));
    gtx::JoinInfo hi;
    rc = hits_pass(c, q, mode, c->join.hitsOut.get(), &hi); if (rc) return rc;                 // (synchronises: qb / iv may go)
    if ((flags & GTX_CHECK_SORTED) && b0 > 0 && acc.first_unsorted < 0) {                         // the seam between two batches, as in join_batches
      const int32_t *p = reads + 3 * (b0 - 1), *r = reads + 3 * b0;
      if (r[0] < p[0] || (r[0] == p[0] && r[1] < p[1])) acc.first_unsorted = b0;
    }
    join_info_merge(&acc, hi, b0);
    HIPCHK(c, hipMemcpy(hits_out + b0, c->join.hitsOut.get(), sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
  }
  if (info) *info = acc;
  return GTX_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// pair offsets (gtx_offset.hip)
// ---------------------------------------------------------------------------------------------

// the per-ordinal reference point (front / back interval) as of gtx_set_ref_blocks
static int offset_prepare(gtx_ctx *c)
{
  if (c->rx.offRef) return GTX_OK;
  const size_t m = (size_t)std::max<int64_t>(c->nRefs, 1);
  std::vector<int2> env(m, make_int2(0, 0));
  for (int64_t k = 0; k < c->nRefs; k++) env[k] = make_int2(c->h_refS[k], c->h_refE[k]);
  DevBuf<int2> d_env;
  HIPCHK(c, d_env.alloc(m));
  HIPCHK(c, c->rx.offRef.alloc(m));
  HIPCHK(c, hipMemcpy(d_env.get(), env.data(), sizeof(int2) * m, hipMemcpyHostToDevice));
  HIPCHK(c, gtx::launch_ref_ends(d_env.get(), ref_blocks(c), c->nRefs, c->rx.offRef.get(), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));                   // (before d_env goes)
  return GTX_OK;
}

static int offset_op(int32_t op) { return op >= GTX_OFFSET_1 && op <= GTX_OFFSET_3P ? op : 0; }

// the offsets of the pairs of queries [q0, q1) into d_out; *inv = the first inverted pair (relative to d_off[q0]), INT64_MAX if none.
// Waits for the stream.
static int pair_offsets(gtx_ctx *c, const gtx::OffsetArgs &a, int64_t q0, int64_t q1, const long long *d_off, const int *d_pairs, int64_t n_pairs,
                        long long *d_out, long long *inv)
{
  const long long none = INT64_MAX;
  HIPCHK(c, hipMemcpyAsync(c->join.offInv.get(), &none, sizeof none, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gtx::launch_pair_offsets(a, q0, q1, d_off, d_pairs, n_pairs, d_out, c->join.offInv.get(), c->join.big.get(), c->stream));
  *inv = INT64_MAX;
  HIPCHK(c, hipMemcpyAsync(inv, c->join.offInv.get(), sizeof *inv, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GTX_OK;
}

extern "C" {

int gtx_set_ref_strands(gtx_ctx *c, const int8_t *strand)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_set_ref_strands: gtx_set_refs has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rx.refStrand.reset();
  if (!strand || c->nRefs == 0) return GTX_OK;
  for (int64_t k = 0; k < c->nRefs; k++)
    if (strand[k] != '+' && strand[k] != '-') return fail(c, GTX_E_ARG, "gtx_set_ref_strands: a strand is '+' or '-'");
  HIPCHK(c, upload(c->rx.refStrand, strand, (size_t)c->nRefs));
  return GTX_OK;
}

int gtx_join_offsets(gtx_ctx *c, const int32_t *reads, const int64_t *first, const int32_t *blocks, const int8_t *read_strands, int64_t n,
                     uint32_t flags, int32_t op, int64_t *offsets_out, int32_t *pairs_out, int64_t cap, int64_t *entry_offsets_out,
                     int64_t *entries_out, int64_t entry_cap, int64_t *first_inverted_out, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_join_offsets: gtx_set_refs has not been called");
  const int o = offset_op(op);
  const bool skip = flags & GTX_OFFSET_SKIP_REF_GAPS, fromQuery = flags & GTX_OFFSET_FROM_QUERY;
  if (!o || (skip && fromQuery) || cap < 0 || (cap > 0 && (!pairs_out || !entry_offsets_out)) || entry_cap < 0 || (entry_cap > 0 && !entries_out))
    return fail(c, GTX_E_ARG, "gtx_join_offsets: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = offset_prepare(c); if (rc) return rc;
  int64_t ebase = 0, inverted = -1, strandsOf = -1;            // entries before the chunk; the first inverted pair; the batch whose strands are up
  if (cap > 0) entry_offsets_out[0] = 0;
  if (!c->join.offInv) HIPCHK(c, c->join.offInv.alloc(1));
  rc = join_batches(c, "gtx_join_offsets", reads, first, blocks, n, flags, true, offsets_out, cap, info,
    [&](const gtx::JoinQueries &q, int64_t b0, int64_t q0, int64_t q1, int64_t p0, int64_t len) -> int {
      int r = GTX_OK;
      const int64_t keep = std::min(len, cap - p0);
      HIPCHK(c, hipMemcpy(pairs_out + p0, c->join.pairs.get(), sizeof(int32_t) * keep, hipMemcpyDeviceToHost));
      gtx::OffsetArgs a{q, nullptr, c->rx.offRef.get(), c->rx.refStrand.get(), ref_blocks(c), o, fromQuery};
      if (fromQuery && read_strands) {
        if (strandsOf != b0) {
          const int64_t m = std::min<int64_t>(n - b0, std::max<int64_t>(1, c->batchReads));
          HIPCHK(c, c->join.offQStrand.grow((size_t)m));
          HIPCHK(c, hipMemcpy(c->join.offQStrand.get(), read_strands + b0, (size_t)m, hipMemcpyHostToDevice));
          strandsOf = b0;
        }
        a.qStrand = c->join.offQStrand.get();
      }
      HIPCHK(c, c->join.big.grow((size_t)(q1 - q0 + 1)));
      int64_t nent = len;
      if (!skip) {
        HIPCHK(c, c->join.offOut.grow((size_t)(2 * len)));
        long long inv;
        r = pair_offsets(c, a, q0, q1, c->join.off.get(), c->join.pairs.get(), len, c->join.offOut.get(), &inv); if (r) return r;
        if (inverted < 0 && inv < keep) inverted = p0 + inv;
        for (int64_t p = 1; p <= keep; p++) entry_offsets_out[p0 + p] = ebase + p;
        nent = keep;
      } else {
        HIPCHK(c, c->join.offCnt.grow((size_t)(len + 1)));
        HIPCHK(c, c->join.offPart.grow((size_t)gtx::join_scan_partials(len + 1)));
        HIPCHK(c, gtx::launch_pair_gaps_count(a, q0, q1, c->join.off.get(), c->join.pairs.get(), len, c->join.offCnt.get(), c->join.big.get(), c->stream));
        HIPCHK(c, hipMemsetAsync(c->join.offCnt.get() + len, 0, sizeof(long long), c->stream));
        HIPCHK(c, gtx::launch_join_scan(c->join.offCnt.get(), len + 1, c->join.offPart.get(), c->stream));
        std::vector<int64_t> eoff((size_t)len + 1);
        HIPCHK(c, hipMemcpyAsync(eoff.data(), c->join.offCnt.get(), sizeof(int64_t) * (len + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nent = eoff[len];
        HIPCHK(c, c->join.offOut.grow((size_t)(2 * nent)));
        if (nent > 0) HIPCHK(c, gtx::launch_pair_gaps_emit(a, q0, q1, c->join.off.get(), c->join.pairs.get(), len, c->join.offCnt.get(), c->join.offOut.get(), c->join.big.get(), c->stream));
        for (int64_t p = 1; p <= keep; p++) entry_offsets_out[p0 + p] = ebase + eoff[p];
        nent = eoff[keep];
      }
      const int64_t ekeep = std::max<int64_t>(0, std::min(nent, entry_cap - ebase));
      if (ekeep > 0) HIPCHK(c, hipMemcpy(entries_out + 2 * ebase, c->join.offOut.get(), sizeof(int64_t) * 2 * ekeep, hipMemcpyDeviceToHost));
      ebase += nent;
      return GTX_OK;
    });
  if (rc) return rc;
  if (first_inverted_out) *first_inverted_out = inverted;
  return GTX_OK;
}

int gtx_pair_offsets_device(gtx_ctx *c, const void *d_reads, int64_t n, const void *d_offsets, const void *d_pairs, int64_t n_pairs, int32_t op,
                            void *d_out, int64_t *first_inverted_out)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_pair_offsets_device: gtx_set_refs has not been called");
  const int o = offset_op(op);
  if (!o || n < 0 || (n > 0 && (!d_reads || !d_offsets)) || n_pairs < 0 || (n_pairs > 0 && (!d_pairs || !d_out)))
    return fail(c, GTX_E_ARG, "gtx_pair_offsets_device: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = offset_prepare(c); if (rc) return rc;
  if (!c->join.offInv) HIPCHK(c, c->join.offInv.alloc(1));
  HIPCHK(c, c->join.big.grow((size_t)(n + 1)));
  const gtx::OffsetArgs a{gtx::JoinQueries{(const int *)d_reads, nullptr, nullptr, n}, nullptr, c->rx.offRef.get(), c->rx.refStrand.get(), ref_blocks(c), o, false};
  long long inv;
  rc = pair_offsets(c, a, 0, n, (const long long *)d_offsets, (const int *)d_pairs, n_pairs, (long long *)d_out, &inv); if (rc) return rc;
  if (first_inverted_out) *first_inverted_out = inv == INT64_MAX ? -1 : inv;
  return GTX_OK;
}

// ---- the annotate pass (gtx_annotate.hip) ----

} // extern "C"

static bool annotate_args(gtx_ctx *c, int64_t n_primary, int32_t op_primary, int32_t op_rest, int32_t mode, const int *d_tri, gtx::AnnotateArgs *a)
{
  if (!offset_op(op_primary) || !offset_op(op_rest) || n_primary < 0 || n_primary > c->nRefs || (mode != GTX_ANNOTATE_CENTER && mode != GTX_ANNOTATE_START)) return false;
  *a = gtx::AnnotateArgs{d_tri, c->rx.offRef.get(), c->rx.refStrand.get(), c->nRefs, n_primary, op_primary, op_rest,
                         mode == GTX_ANNOTATE_CENTER ? gtx::ANN_CENTER : gtx::ANN_START};
  return true;
}

// count, scan and emit over the pairs of queries [q0, q1): d_cnt (q1 - q0 + 1) becomes the kept offsets from 0, *kept their total;
// the kept pairs below cap go to d_ref / d_val.  Waits for the stream.
static int annotate_pass(gtx_ctx *c, const gtx::AnnotateArgs &a, int64_t q0, int64_t q1, const long long *d_off, const int *d_pairs, int64_t n_pairs,
                         long long *d_cnt, int *d_ref, long long *d_val, int64_t cap, int64_t *kept)
{
  const int64_t m = q1 - q0;
  HIPCHK(c, c->join.big.grow((size_t)(m + 1)));
  HIPCHK(c, c->join.offPart.grow((size_t)gtx::join_scan_partials(m + 1)));
  HIPCHK(c, gtx::launch_annotate_count(a, q0, q1, d_off, d_pairs, n_pairs, d_cnt, c->join.big.get(), c->stream));
  HIPCHK(c, hipMemsetAsync(d_cnt + m, 0, sizeof(long long), c->stream));
  HIPCHK(c, gtx::launch_join_scan(d_cnt, m + 1, c->join.offPart.get(), c->stream));
  HIPCHK(c, gtx::launch_annotate_emit(a, q0, q1, d_off, d_pairs, n_pairs, d_cnt, d_ref, d_val, cap, c->join.big.get(), c->stream));
  long long t = 0;
  HIPCHK(c, hipMemcpyAsync(&t, d_cnt + m, sizeof t, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *kept = t;
  return GTX_OK;
}

extern "C" {

int gtx_pair_annotate_device(gtx_ctx *c, const void *d_reads, int64_t n, const void *d_offsets, const void *d_pairs, int64_t n_pairs, int64_t n_primary,
                             int32_t op_primary, int32_t op_rest, int32_t mode, void *d_kept_offsets, void *d_kept_ref, void *d_kept_value,
                             int64_t cap, int64_t *n_kept_out)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_pair_annotate_device: gtx_set_refs has not been called");
  gtx::AnnotateArgs a;
  if (n < 0 || !d_kept_offsets || (n > 0 && (!d_reads || !d_offsets)) || n_pairs < 0 || (n_pairs > 0 && !d_pairs) || cap < 0 ||
      (cap > 0 && (!d_kept_ref || !d_kept_value)) || !annotate_args(c, n_primary, op_primary, op_rest, mode, (const int *)d_reads, &a))
    return fail(c, GTX_E_ARG, "gtx_pair_annotate_device: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = offset_prepare(c); if (rc) return rc;
  a.refEnds = c->rx.offRef.get();
  int64_t kept = 0;
  if (n == 0) HIPCHK(c, hipMemsetAsync(d_kept_offsets, 0, sizeof(long long), c->stream));
  rc = annotate_pass(c, a, 0, n, (const long long *)d_offsets, (const int *)d_pairs, n_pairs, (long long *)d_kept_offsets, (int *)d_kept_ref,
                     (long long *)d_kept_value, cap, &kept); if (rc) return rc;
  if (n_kept_out) *n_kept_out = kept;
  return GTX_OK;
}

int gtx_join_annotate(gtx_ctx *c, const int32_t *reads, int64_t n, uint32_t flags, int64_t n_primary, int32_t op_primary, int32_t op_rest, int32_t mode,
                      int64_t *kept_offsets_out, int32_t *kept_ref_out, int64_t *kept_value_out, int64_t cap, int64_t *n_pairs_out, gtx_count_info *info)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_join_annotate: gtx_set_refs has not been called");
  gtx::AnnotateArgs a;
  if (!kept_offsets_out || cap < 0 || (cap > 0 && (!kept_ref_out || !kept_value_out)) || !annotate_args(c, n_primary, op_primary, op_rest, mode, nullptr, &a))
    return fail(c, GTX_E_ARG, "gtx_join_annotate: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = offset_prepare(c); if (rc) return rc;
  a.refEnds = c->rx.offRef.get();
  std::vector<int64_t> off((size_t)std::max<int64_t>(n, 0) + 1, 0), koff;
  int64_t kbase = 0, done = 0;                                 // kept pairs before the chunk; queries whose kept offsets are written
  kept_offsets_out[0] = 0;
  rc = join_batches(c, "gtx_join_annotate", reads, nullptr, nullptr, n, flags, false, off.data(), INT64_MAX, info,
    [&](const gtx::JoinQueries &q, int64_t b0, int64_t q0, int64_t q1, int64_t, int64_t len) -> int {
      const int64_t m = q1 - q0;
      for (; done < b0 + q0; done++) kept_offsets_out[done + 1] = kbase;      // (queries in front of the chunk that had no pair)
      a.tri = q.tri;
      const int64_t room = std::max<int64_t>(0, std::min(len, cap - kbase));
      HIPCHK(c, c->join.annCnt.grow((size_t)(m + 1)));
      HIPCHK(c, c->join.annRef.grow((size_t)std::max<int64_t>(room, 1)));
      HIPCHK(c, c->join.annVal.grow((size_t)std::max<int64_t>(room, 1)));
      int64_t kept = 0;
      int r = annotate_pass(c, a, q0, q1, c->join.off.get(), c->join.pairs.get(), len, c->join.annCnt.get(), c->join.annRef.get(), c->join.annVal.get(), room, &kept);
      if (r) return r;
      koff.resize((size_t)m + 1);
      HIPCHK(c, hipMemcpy(koff.data(), c->join.annCnt.get(), sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost));
      for (int64_t i = 1; i <= m; i++) kept_offsets_out[b0 + q0 + i] = kbase + koff[i];
      done = b0 + q1;
      const int64_t take = std::min(kept, room);
      if (take > 0) {
        HIPCHK(c, hipMemcpy(kept_ref_out + kbase, c->join.annRef.get(), sizeof(int32_t) * take, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(kept_value_out + kbase, c->join.annVal.get(), sizeof(int64_t) * take, hipMemcpyDeviceToHost));
      }
      kbase += kept;
      return GTX_OK;
    });
  if (rc) return rc;
  for (; done < n; done++) kept_offsets_out[done + 1] = kbase;
  if (n_pairs_out) *n_pairs_out = off[(size_t)std::max<int64_t>(n, 0)];
  return GTX_OK;
}

int gtx_set_signal_bins(gtx_ctx *c, double bin_min, double bin_max, int64_t n_bins, const int64_t *ref_len)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_set_signal_bins: gtx_set_refs has not been called");
  if (n_bins < 0 || n_bins >= INT32_MAX) return fail(c, GTX_E_ARG, "gtx_set_signal_bins: n_bins must lie in [0, 2^31 - 1)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rx.sigRefLen.reset();
  if (ref_len && c->nRefs > 0) HIPCHK(c, upload(c->rx.sigRefLen, (const long long *)ref_len, (size_t)c->nRefs));
  c->rx.sigMin = bin_min; c->rx.sigMax = bin_max; c->rx.sigBins = n_bins; c->rx.sigSet = true;
  return GTX_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// signal bins (gtx_signal.hip)
// ---------------------------------------------------------------------------------------------

static const uint32_t kSignalFlags = GTX_ZERO_LENGTH_OK | GTX_JOIN_GAPS | GTX_SIGNAL_PER_REF | GTX_READS_SORTED | GTX_READS_UNSORTED;

// the index, the reference points and the info block of a call; a = everything but the reads and their weights
static int signal_prepare(gtx_ctx *c, const char *who, uint32_t flags, gtx::SignalArgs &a)
{
  const std::string w(who);
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, (w + ": gtx_set_refs has not been called").c_str());
  if (!c->rx.sigSet) return fail(c, GTX_E_STATE, (w + ": gtx_set_signal_bins has not been called").c_str());
  if (flags & ~kSignalFlags) return fail(c, GTX_E_ARG, (w + ": unknown flag").c_str());
  HIPCHK(c, hipSetDevice(c->device));
  int rc = join_prepare(c); if (rc) return rc;
  rc = offset_prepare(c); if (rc) return rc;
  if (!c->sig.info) HIPCHK(c, c->sig.info.alloc(1));
  a = gtx::SignalArgs{};
  a.ix = c->rx.pairAll.ix;
  a.rb = ref_blocks(c);
  a.mode = join_mode(c, flags & (GTX_ZERO_LENGTH_OK | GTX_JOIN_GAPS));
  a.refEnds = c->rx.offRef.get(); a.refStrand = (const signed char *)c->rx.refStrand.get(); a.refLen = c->rx.sigRefLen.get();
  a.binMin = c->rx.sigMin; a.binMax = c->rx.sigMax; a.nBins = c->rx.sigBins;
  a.perRef = (flags & GTX_SIGNAL_PER_REF) != 0;
  return GTX_OK;
}

static int64_t signal_len(const gtx_ctx *c, uint32_t flags) { return ((flags & GTX_SIGNAL_PER_REF) ? std::max<int64_t>(c->nRefs, 0) : 1) * c->rx.sigBins; }
static int signal_cus(const gtx_ctx *c) { return (int)std::max<int64_t>(1, c->waveSlots / 32); }

// the signal pass of a.q into d_bins with a fresh info block, then that block into *info / *firstInv (read indices from base);
// waits for the stream
static int signal_pass(gtx_ctx *c, const gtx::SignalArgs &a, unsigned long long *d_bins, gtx_signal_info *info, long long *firstInv, int64_t base)
{
  const gtx::SignalInfo init = {0, 0, 0, 0, 0, 0, INT64_MAX};
  HIPCHK(c, hipMemcpyAsync(c->sig.info.get(), &init, sizeof init, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gtx::launch_signal_bins(a, d_bins, c->sig.info.get(), signal_cus(c), c->stream));
  gtx::SignalInfo h;
  HIPCHK(c, hipMemcpyAsync(&h, c->sig.info.get(), sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (info) {
    info->n_pairs += (int64_t)h.pairs; info->n_binned += (int64_t)h.binned; info->n_dropped += (int64_t)h.dropped;
    info->weight_abs_sum += (int64_t)h.absWeight; info->n_no_class += (int64_t)h.noClass; info->n_degenerate += (int64_t)h.degenerate;
  }
  if (h.firstInverted != INT64_MAX && *firstInv < 0) *firstInv = h.firstInverted + base;
  return GTX_OK;
}

extern "C" {

int gtx_signal_bins_device(gtx_ctx *c, const void *d_reads, const void *d_weights, int64_t n, uint32_t flags, void *d_bins,
                           int64_t *first_inverted_out, gtx_signal_info *info)
{
  if (!c) return GTX_E_ARG;
  gtx::SignalArgs a;
  int rc = signal_prepare(c, "gtx_signal_bins_device", flags, a); if (rc) return rc;
  if (n < 0 || (n > 0 && !d_reads) || (signal_len(c, flags) > 0 && !d_bins)) return fail(c, GTX_E_ARG, "gtx_signal_bins_device: bad argument");
  a.q = gtx::JoinQueries{(const int *)d_reads, nullptr, nullptr, n};
  a.w = (const long long *)d_weights;
  if (info) memset(info, 0, sizeof *info);
  long long inv = -1;
  rc = signal_pass(c, a, (unsigned long long *)d_bins, info, &inv, 0); if (rc) return rc;
  if (first_inverted_out) *first_inverted_out = inv;
  return GTX_OK;
}

int gtx_signal_bins(gtx_ctx *c, const int32_t *reads, const int64_t *first, const int32_t *blocks, const int64_t *weights, int64_t n,
                    uint32_t flags, int64_t *bins_out, int64_t *first_inverted_out, gtx_signal_info *info)
{
  if (!c) return GTX_E_ARG;
  gtx::SignalArgs a;
  int rc = signal_prepare(c, "gtx_signal_bins", flags, a); if (rc) return rc;
  const int64_t len = signal_len(c, flags);
  if ((len > 0 && !bins_out) || !queries_ok(reads, first, blocks, n)) return fail(c, GTX_E_ARG, "gtx_signal_bins: bad argument");
  if (info) memset(info, 0, sizeof *info);
  HIPCHK(c, c->sig.bins.grow((size_t)std::max<int64_t>(len, 1)));
  HIPCHK(c, hipMemsetAsync(c->sig.bins.get(), 0, sizeof(unsigned long long) * (size_t)std::max<int64_t>(len, 1), c->stream));
  long long inv = -1;
  const int64_t per = std::max<int64_t>(1, c->batchReads);
  const std::string who("gtx_signal_bins");
  for (int64_t b0 = 0; b0 < n; b0 += per) {
    const int64_t b1 = std::min(n, b0 + per), m = b1 - b0;
    std::vector<int2> qb, iv;
    rc = stage_queries(c, who, reads, first, blocks, b0, b1, true, qb, iv, a.q); if (rc) return rc;
    a.w = nullptr;
    if (weights) {
      HIPCHK(c, c->sig.w.grow((size_t)m));
      HIPCHK(c, hipMemcpyAsync(c->sig.w.get(), weights + b0, sizeof(int64_t) * m, hipMemcpyHostToDevice, c->stream));
      a.w = c->sig.w.get();
    }
    rc = signal_pass(c, a, c->sig.bins.get(), info, &inv, b0); if (rc) return rc;          // (synchronises: qb / iv may go)
  }
  if (len > 0) {
    std::vector<int64_t> h((size_t)len);
    HIPCHK(c, hipMemcpy(h.data(), c->sig.bins.get(), sizeof(int64_t) * (size_t)len, hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < len; k++) bins_out[k] = (int64_t)((uint64_t)bins_out[k] + (uint64_t)h[k]);
  }
  if (first_inverted_out) *first_inverted_out = inv;
  return GTX_OK;
}

} // extern "C"
