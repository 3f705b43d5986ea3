// gtx_api_link.hip -- the C ABI's passes over one sorted region set: link (gtx_link*) and the neighbour passes (gtx_adjacent*,
// gtx_gaps*).  Host code only (the kernels: gtx_link.hip, gtx_adjacent.hip); the context and the helpers shared with the other
// families are in gtx_ctx.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include "gtx.h"
#include "gtx_link.h"
#include "gtx_adjacent.h"
#include "gtx_ctx.h"

extern "C" {

// ---------------------------------------------------------------------------------------------
// link (kernels: gtx_link.hip)
// ---------------------------------------------------------------------------------------------
static int link_mode(uint32_t flags, bool haveValues, int *mode)
{
  const uint32_t f = flags & (GTX_LINK_SUM | GTX_LINK_MIN | GTX_LINK_MAX);
  if (flags & ~(GTX_LINK_SUM | GTX_LINK_MIN | GTX_LINK_MAX)) return GTX_E_ARG;
  if (f & (f - 1)) return GTX_E_ARG;                                 // at most one fold
  if (f && !haveValues) return GTX_E_ARG;
  *mode = f == GTX_LINK_SUM ? gtx::LINK_SUM : f == GTX_LINK_MIN ? gtx::LINK_MIN : f == GTX_LINK_MAX ? gtx::LINK_MAX : gtx::LINK_NONE;
  return GTX_OK;
}

// the info block of a gtx_link_device call that has not been synchronised yet goes to its caller's struct before the page-locked
// block is used again
static int link_settle(gtx_ctx *c)
{
  if (!c->link.mail.pending) return GTX_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->link.mail.deliver();
  return GTX_OK;
}

// the kernels and the copy of the info block into page-locked memory, enqueued
static int link_enqueue(gtx_ctx *c, const void *d_tri, const void *d_vals, int64_t n, int64_t d, int mode, void *d_head, void *d_cnt, void *d_stop, void *d_val)
{
  const size_t nt = (size_t)gtx::link_tiles(n);
  HIPCHK(c, c->link.agg.reserve(nt)); HIPCHK(c, c->link.prefix.reserve(nt)); HIPCHK(c, c->link.bits.reserve(nt * (gtx::kLinkTile / 64) + 1));
  HIPCHK(c, c->link.heads.reserve(nt)); HIPCHK(c, c->link.base.reserve(nt + 1));
  HIPCHK(c, c->link.mail.ready());
  gtx::LinkWork w;
  w.tileAgg = c->link.agg.get(); w.tilePrefix = c->link.prefix.get(); w.bits = c->link.bits.get(); w.tileHeads = c->link.heads.get();
  w.tileHeadBase = c->link.base.get(); w.info = c->link.mail.dev.get();
  HIPCHK(c, gtx::launch_link((const int *)d_tri, (const long long *)d_vals, n, d, mode, w, (unsigned *)d_head, (unsigned *)d_cnt, (int *)d_stop,
                             (long long *)d_val, c->stream));
  HIPCHK(c, c->link.mail.post(c->stream));
  return GTX_OK;
}

int gtx_link_device(gtx_ctx *c, const void *d_triples, const void *d_values, int64_t n, int64_t max_difference, uint32_t flags,
                    void *d_head, void *d_count, void *d_stop, void *d_value, gtx_link_info *info)
{
  if (!c) return GTX_E_ARG;
  int mode = 0;
  if (link_mode(flags, d_values != nullptr && d_value != nullptr, &mode)) return fail(c, GTX_E_ARG, "gtx_link_device: at most one of GTX_LINK_SUM / _MIN / _MAX, and values with it");
  if (n < 0 || n >= (1ll << 32) || !info || (n > 0 && (!d_triples || !d_head || !d_count || !d_stop))) return fail(c, GTX_E_ARG, "gtx_link_device: bad argument (n < 2^32)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = link_settle(c); if (rc) return rc; }
  info->n_groups = 0; info->first_unsorted = -1;
  if (n == 0) return GTX_OK;
  if (int rc = link_enqueue(c, d_triples, d_values, n, max_difference, mode, d_head, d_count, d_stop, d_value)) return rc;
  c->link.mail.pending = info;
  return GTX_OK;
}

int gtx_link(gtx_ctx *c, const int32_t *triples, const int64_t *values, int64_t n, int64_t max_difference, uint32_t flags,
             uint32_t *head_out, uint32_t *count_out, int32_t *stop_out, int64_t *value_out, gtx_link_info *info)
{
  if (!c) return GTX_E_ARG;
  int mode = 0;
  if (link_mode(flags, values != nullptr && value_out != nullptr, &mode)) return fail(c, GTX_E_ARG, "gtx_link: at most one of GTX_LINK_SUM / _MIN / _MAX, and values with it");
  if (n < 0 || n >= (1ll << 32) || !info || (n > 0 && (!triples || !head_out || !count_out || !stop_out))) return fail(c, GTX_E_ARG, "gtx_link: bad argument (n < 2^32)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = link_settle(c); if (rc) return rc; }
  info->n_groups = 0; info->first_unsorted = -1;
  if (n == 0) return GTX_OK;
  const size_t m = (size_t)n;
  HIPCHK(c, c->link.tri.reserve(3 * m)); HIPCHK(c, c->link.head.reserve(m)); HIPCHK(c, c->link.cnt.reserve(m)); HIPCHK(c, c->link.stop.reserve(m));
  if (mode) { HIPCHK(c, c->link.vals.reserve(m)); HIPCHK(c, c->link.val.reserve(m)); }
  HIPCHK(c, hipMemcpyAsync(c->link.tri.get(), triples, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, c->stream));
  if (mode) HIPCHK(c, hipMemcpyAsync(c->link.vals.get(), values, sizeof(int64_t) * m, hipMemcpyHostToDevice, c->stream));
  if (int rc = link_enqueue(c, c->link.tri.get(), mode ? c->link.vals.get() : nullptr, n, max_difference, mode, c->link.head.get(), c->link.cnt.get(),
                            c->link.stop.get(), mode ? c->link.val.get() : nullptr)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const gtx::LinkInfo &h = c->link.mail.host.get()[0];
  publish(h, info);
  const size_t g = (size_t)h.nGroups;
  if (g) {
    HIPCHK(c, hipMemcpyAsync(head_out, c->link.head.get(), sizeof(uint32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(count_out, c->link.cnt.get(), sizeof(uint32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(stop_out, c->link.stop.get(), sizeof(int32_t) * g, hipMemcpyDeviceToHost, c->stream));
    if (mode) HIPCHK(c, hipMemcpyAsync(value_out, c->link.val.get(), sizeof(int64_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GTX_OK;
}

// link fed as a stream of text blocks (the tool's path): see include/gtx.h
int gtx_link_text_begin(gtx_ctx *c, int32_t n_chrom, int sorted_by_strand, int64_t capacity)
{
  if (!c) return GTX_E_ARG;
  if (n_chrom < 0 || capacity < 0 || capacity >= (1ll << 32)) return fail(c, GTX_E_ARG, "gtx_link_text_begin: bad argument (capacity < 2^32)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = link_settle(c); if (rc) return rc; }
  HIPCHK(c, c->link.textTri.reserve(3 * (size_t)std::max<int64_t>(capacity, 1))); HIPCHK(c, c->link.minus.reserve((size_t)std::max<int64_t>(capacity, 1)));
  c->link.textOpen = true; c->link.textN = 0; c->link.textCap = capacity; c->link.textChrom = n_chrom; c->link.textByStrand = sorted_by_strand != 0;
  return GTX_OK;
}

int gtx_link_add_text(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, int *needs_host)
{
  if (!c) return GTX_E_ARG;
  if (!c->link.textOpen) return fail(c, GTX_E_STATE, "gtx_link_add_text: gtx_link_text_begin has not been called");
  if (!text || !r || !needs_host || nLines < 0 || bytes >= (1ull << 32) - 4096 || nLines >= (1ll << 31) || r->n_chrom != c->link.textChrom || (r->n_chrom > 0 && !r->chrom_names) ||
      !r->strand_aware || r->sorted_rules || r->max_label_value > 1 || c->link.textN + nLines > c->link.textCap)
    return fail(c, GTX_E_ARG, "gtx_link_add_text: bad argument (strand-aware rules without order or label rules, the names of gtx_link_text_begin, room for the lines)");
  *needs_host = 0;
  TextSlot *tp = nullptr; bool empty = false; int ticket = 0;
  // (the sorted scanner's rules: nothing about the interval is checked -- zero-length and inverted regions are link's to take)
  { int rc = text_stage(c, text, bytes, nLines, r, false, 2, nullptr, 0, &tp, &ticket, &empty); if (rc || empty) return rc; }
  TextSlot &t = *tp;
  HIPCHK(c, gtx::launch_link_append(t.tri.get(), nLines, c->link.textChrom, c->link.textByStrand, c->link.textTri.get() + 3 * c->link.textN,
                                    c->link.minus.get() + c->link.textN, t.flag.get(), c->stream));
  HIPCHK(c, hipMemcpyAsync(t.hostFlag.get(), t.flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(t.evParsed, c->stream));
  HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
  t.busy = true;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (*t.hostFlag.get()) { *needs_host = 1; return GTX_OK; }           // (what was appended lies behind the end and is written over)
  c->link.textN += nLines;
  return GTX_OK;
}

int gtx_link_add(gtx_ctx *c, const int32_t *triples, const uint8_t *minus, int64_t n)
{
  if (!c) return GTX_E_ARG;
  if (!c->link.textOpen) return fail(c, GTX_E_STATE, "gtx_link_add: gtx_link_text_begin has not been called");
  if (n < 0 || (n > 0 && (!triples || !minus)) || c->link.textN + n > c->link.textCap) return fail(c, GTX_E_ARG, "gtx_link_add: bad argument");
  if (n == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->link.textTri.get() + 3 * c->link.textN, triples, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->link.minus.get() + c->link.textN, minus, (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->link.textN += n;
  return GTX_OK;
}

int gtx_link_text_end(gtx_ctx *c, int64_t max_difference, uint32_t *head_out, int32_t *stop_out, int32_t *head_key_out, gtx_link_info *info)
{
  if (!c) return GTX_E_ARG;
  if (!c->link.textOpen) return fail(c, GTX_E_STATE, "gtx_link_text_end: gtx_link_text_begin has not been called");
  c->link.textOpen = false;
  const int64_t n = c->link.textN;
  if (!info || (n > 0 && (!head_out || !stop_out || !head_key_out))) return fail(c, GTX_E_ARG, "gtx_link_text_end: bad argument");
  info->n_groups = 0; info->first_unsorted = -1;
  if (n == 0) return GTX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t m = (size_t)n;
  HIPCHK(c, c->link.head.reserve(m)); HIPCHK(c, c->link.cnt.reserve(m)); HIPCHK(c, c->link.stop.reserve(m)); HIPCHK(c, c->link.headKey.reserve(m));
  if (int rc = link_enqueue(c, c->link.textTri.get(), nullptr, n, max_difference, gtx::LINK_NONE, c->link.head.get(), c->link.cnt.get(), c->link.stop.get(), nullptr)) return rc;
  HIPCHK(c, gtx::launch_link_head_keys(c->link.textTri.get(), c->link.minus.get(), c->link.head.get(), c->link.mail.dev.get(), n, c->link.textByStrand, c->link.headKey.get(), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const gtx::LinkInfo &h = c->link.mail.host.get()[0];
  publish(h, info);
  const size_t g = (size_t)h.nGroups;
  if (g) {
    HIPCHK(c, hipMemcpyAsync(head_out, c->link.head.get(), sizeof(uint32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(stop_out, c->link.stop.get(), sizeof(int32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(head_key_out, c->link.headKey.get(), sizeof(int2) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GTX_OK;
}

// ---------------------------------------------------------------------------------------------
// the neighbour passes (kernels: gtx_adjacent.hip)
// ---------------------------------------------------------------------------------------------
// the info blocks of device calls that have not been synchronised yet go to their callers' structs before a page-locked block is
// used again
static int adjacent_settle(gtx_ctx *c)
{
  if (!c->nbr.adj.pending && !c->nbr.gap.pending) return GTX_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->nbr.adj.deliver(); c->nbr.gap.deliver();
  return GTX_OK;
}

static int adjacent_enqueue(gtx_ctx *c, const void *d_tri, const void *d_minus, int64_t n, int op1, int op2, void *d_dist)
{
  HIPCHK(c, c->nbr.sums.reserve((size_t)gtx::adjacent_tiles(n)));
  HIPCHK(c, c->nbr.adj.ready());
  HIPCHK(c, gtx::launch_adjacent((const int *)d_tri, (const unsigned char *)d_minus, n, op1, op2, (long long *)d_dist, c->nbr.sums.get(), c->nbr.adj.dev.get(), c->stream));
  HIPCHK(c, c->nbr.adj.post(c->stream));
  return GTX_OK;
}

static bool adjacent_args_ok(int64_t n, int op1, int op2, const void *tri, const void *info)
{
  return n >= 0 && n < (1ll << 32) && op1 >= GTX_POINT_START && op1 <= GTX_POINT_3P && op2 >= GTX_POINT_START && op2 <= GTX_POINT_3P && info && (n == 0 || tri);
}

int gtx_adjacent_device(gtx_ctx *c, const void *d_triples, const void *d_minus, int64_t n, int op1, int op2, void *d_dist, gtx_adjacent_info *info)
{
  if (!c) return GTX_E_ARG;
  if (!adjacent_args_ok(n, op1, op2, d_triples, info)) return fail(c, GTX_E_ARG, "gtx_adjacent_device: bad argument (n < 2^32, points 0..3)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = adjacent_settle(c); if (rc) return rc; }
  info->first_unsorted = -1; info->n_inclusions = 0; info->n_overlaps = 0;
  if (n == 0) return GTX_OK;
  if (int rc = adjacent_enqueue(c, d_triples, d_minus, n, op1, op2, d_dist)) return rc;
  c->nbr.adj.pending = info;
  return GTX_OK;
}

int gtx_adjacent(gtx_ctx *c, const int32_t *triples, const uint8_t *minus, int64_t n, int op1, int op2, int64_t *dist_out, gtx_adjacent_info *info)
{
  if (!c) return GTX_E_ARG;
  if (!adjacent_args_ok(n, op1, op2, triples, info)) return fail(c, GTX_E_ARG, "gtx_adjacent: bad argument (n < 2^32, points 0..3)");
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = adjacent_settle(c); if (rc) return rc; }
  info->first_unsorted = -1; info->n_inclusions = 0; info->n_overlaps = 0;
  if (n == 0) return GTX_OK;
  const size_t m = (size_t)n;
  const bool strands = minus != nullptr && dist_out != nullptr;
  HIPCHK(c, c->nbr.tri.reserve(3 * m));
  if (strands) HIPCHK(c, c->nbr.minus.reserve(m));
  if (dist_out) HIPCHK(c, c->nbr.dist.reserve(m));
  HIPCHK(c, hipMemcpyAsync(c->nbr.tri.get(), triples, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, c->stream));
  if (strands) HIPCHK(c, hipMemcpyAsync(c->nbr.minus.get(), minus, m, hipMemcpyHostToDevice, c->stream));
  if (int rc = adjacent_enqueue(c, c->nbr.tri.get(), strands ? c->nbr.minus.get() : nullptr, n, op1, op2, dist_out ? c->nbr.dist.get() : nullptr)) return rc;
  if (dist_out) HIPCHK(c, hipMemcpyAsync(dist_out, c->nbr.dist.get(), sizeof(int64_t) * m, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  publish(c->nbr.adj.host.get()[0], info);
  return GTX_OK;
}

// the arguments of both gap entries; the bounds go to the device here (they are host memory in both)
static int gaps_prepare(gtx_ctx *c, const char *who, const void *tri, int64_t n, const int64_t *bounds, int32_t n_bounds, int64_t capacity, const void *owner,
                        const void *start, const void *stop, gtx_gaps_info *info)
{
  if (n < 0 || n >= (1ll << 32) || n_bounds < 0 || (n_bounds > 0 && !bounds) || capacity < 0 || !info || (n > 0 && !tri) || (capacity > 0 && (!owner || !start || !stop)))
    return fail(c, GTX_E_ARG, (std::string(who) + ": bad argument (n < 2^32)").c_str());
  for (int32_t k = 0; k < n_bounds; k++)
    if (bounds[k] > (int64_t)INT32_MAX - 2) return fail(c, GTX_E_RANGE, (std::string(who) + ": a bound above 2^31 - 3").c_str());
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = adjacent_settle(c); if (rc) return rc; }
  info->n_gaps = 0; info->first_bad = -1; info->bad_kind = 0;
  if (n == 0) return GTX_OK;
  HIPCHK(c, c->nbr.gapBounds.reserve((size_t)std::max<int32_t>(n_bounds, 1)));
  if (n_bounds > 0) HIPCHK(c, hipMemcpyAsync(c->nbr.gapBounds.get(), bounds, sizeof(int64_t) * (size_t)n_bounds, hipMemcpyHostToDevice, c->stream));
  const size_t ns = (size_t)gtx::adjacent_spans(n);
  HIPCHK(c, c->nbr.gapCount.reserve(ns)); HIPCHK(c, c->nbr.gapBase.reserve(ns + 1));
  HIPCHK(c, c->nbr.gap.ready());
  return GTX_OK;
}

static int gaps_enqueue(gtx_ctx *c, const void *d_tri, int64_t n, int32_t n_bounds, int64_t capacity, void *d_owner, void *d_start, void *d_stop)
{
  HIPCHK(c, gtx::launch_gaps((const int *)d_tri, n, c->nbr.gapBounds.get(), n_bounds, capacity, c->nbr.gapCount.get(), c->nbr.gapBase.get(), c->nbr.gap.dev.get(), (unsigned *)d_owner,
                             (int *)d_start, (int *)d_stop, c->stream));
  HIPCHK(c, c->nbr.gap.post(c->stream));
  return GTX_OK;
}

int gtx_gaps_device(gtx_ctx *c, const void *d_triples, int64_t n, const int64_t *bounds, int32_t n_bounds, int64_t capacity, void *d_owner, void *d_start, void *d_stop,
                    gtx_gaps_info *info)
{
  if (!c) return GTX_E_ARG;
  if (int rc = gaps_prepare(c, "gtx_gaps_device", d_triples, n, bounds, n_bounds, capacity, d_owner, d_start, d_stop, info)) return rc;
  if (n == 0) return GTX_OK;
  if (int rc = gaps_enqueue(c, d_triples, n, n_bounds, capacity, d_owner, d_start, d_stop)) return rc;
  c->nbr.gap.pending = info;
  return GTX_OK;
}

int gtx_gaps(gtx_ctx *c, const int32_t *triples, int64_t n, const int64_t *bounds, int32_t n_bounds, int64_t capacity, uint32_t *owner_out, int32_t *start_out,
             int32_t *stop_out, gtx_gaps_info *info)
{
  if (!c) return GTX_E_ARG;
  if (int rc = gaps_prepare(c, "gtx_gaps", triples, n, bounds, n_bounds, capacity, owner_out, start_out, stop_out, info)) return rc;
  if (n == 0) return GTX_OK;
  const size_t m = (size_t)n, cap = (size_t)std::max<int64_t>(capacity, 1);
  HIPCHK(c, c->nbr.tri.reserve(3 * m)); HIPCHK(c, c->nbr.gapOwner.reserve(cap)); HIPCHK(c, c->nbr.gapStart.reserve(cap)); HIPCHK(c, c->nbr.gapStop.reserve(cap));
  HIPCHK(c, hipMemcpyAsync(c->nbr.tri.get(), triples, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, c->stream));
  if (int rc = gaps_enqueue(c, c->nbr.tri.get(), n, n_bounds, capacity, c->nbr.gapOwner.get(), c->nbr.gapStart.get(), c->nbr.gapStop.get())) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const gtx::GapInfo &h = c->nbr.gap.host.get()[0];
  publish(h, info);
  const size_t g = (size_t)std::min<int64_t>(h.nGaps, capacity);
  if (g) {
    HIPCHK(c, hipMemcpyAsync(owner_out, c->nbr.gapOwner.get(), sizeof(uint32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(start_out, c->nbr.gapStart.get(), sizeof(int32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(stop_out, c->nbr.gapStop.get(), sizeof(int32_t) * g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GTX_OK;
}

} // extern "C"
