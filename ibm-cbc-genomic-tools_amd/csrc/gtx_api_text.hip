// gtx_api_text.hip -- the C ABI's text feed: blocks of region text (BED, SAM, GFF) tokenised on the device and counted, covered or scanned
// where the triples are (gtx_*_add_text), the subset of a block's lines by their hits (gtx_subset_*), their columns rewritten
// (gtx_rewrite_*), their sliding windows (gtx_windows_*) and their conversion to BED or REG lines (gtx_convert_*).  Host code only
// (the kernels: gtx_text.hip, gtx_rewrite.hip, gtx_windows.hip, gtx_convert.hip); the context and the helpers shared with the other
// families are in gtx_ctx.h, the handshake of the entry points that hand text back under a ticket in gtx_api_textblock.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>
#include "gtx.h"
#include "gtx_kernels.h"
#include "gtx_join.h"
#include "gtx_query.h"
#include "gtx_text.h"
#include "gtx_rewrite.h"
#include "gtx_windows.h"
#include "gtx_convert.h"
#include "gtx_ctx.h"
#include "gtx_api_textblock.h"

// ---------------------------------------------------------------------------------------------
// region text tokenised on the device (gtx_text.hip)
// ---------------------------------------------------------------------------------------------
enum TextMode { TEXT_COUNT, TEXT_COVER, TEXT_SCAN };

// A block of text into the slot whose turn it is, and tokenised there (launch_tokenize enqueued on the context's stream): the front
// of add_text and gtx_subset_text.  grouped: the strand-aware outputs (tri2 / w2) are made too when the rules are strand-aware.
// format: launch_tokenize's number, or -1 for the newline index alone (launch_newline_index; gtx_api_blocks.hip).
// *tp = the slot, *ticket its number; *empty: a block without lines -- nothing was enqueued but the slot's evParsed, its verdict is 0.
int text_stage(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, bool grouped, int scanRules,
               unsigned long long *labelSum, int format, TextSlot **tp, int *ticket, bool *empty)
{
  HIPCHK(c, hipSetDevice(c->device));
  const int slot = (int)(c->text.seq & 1);
  TextSlot &t = c->text.slot[slot];
  *ticket = slot; *tp = &t; *empty = false;
  if (!t.evParsed) {
    HIPCHK(c, hipEventCreateWithFlags(&t.evParsed, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&t.evConsumed, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&t.evCopied, hipEventDisableTiming));
    HIPCHK(c, t.flag.alloc(1)); HIPCHK(c, t.hostFlag.alloc(1)); HIPCHK(c, t.seam.alloc(4096));
    HIPCHK(c, t.sum.alloc(1)); HIPCHK(c, hipMemset(t.sum.get(), 0, sizeof(unsigned long long)));
  }
  if (t.busy) { HIPCHK(c, hipEventSynchronize(t.evConsumed)); t.busy = false; }          // the block before last has been counted: its buffers are free
  c->text.seq++;
  if (nLines == 0 || bytes == 0) { *t.hostFlag.get() = 0; HIPCHK(c, hipEventRecord(t.evParsed, c->stream)); *empty = true; return GTX_OK; }
  const size_t nSeg = (bytes + 1023) / 1024;
  if (bytes + 128 > t.text.cap) HIPCHK(c, t.text.alloc(bytes + (bytes >> 3) + 4096));              // (128 bytes beyond the block kept free)
  if (nSeg + 4 > t.seg.cap) HIPCHK(c, t.seg.alloc(nSeg + (nSeg >> 3) + 16));
  if ((size_t)nLines > t.w.cap) {
    t.nl.reset(); t.tri.reset(); t.w.reset();
    const size_t cap = (size_t)nLines + ((size_t)nLines >> 3) + 1024;
    HIPCHK(c, t.nl.alloc(cap)); HIPCHK(c, t.tri.alloc(3 * cap)); HIPCHK(c, t.w.alloc(cap));
  }
  // the names' tables: per set of names (rebuilt when they change)
  {
    std::string blob; std::vector<int32_t> table; unsigned mask = 0;
    size_t total = 0; for (int i = 0; i < r->n_chrom; i++) total += strlen(r->chrom_names[i]) + 1;
    std::string key; key.reserve(total);
    for (int i = 0; i < r->n_chrom; i++) { key += r->chrom_names[i]; key += '\n'; }
    if (key != c->text.blob || !c->text.names) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      gtxtext::build_tables(*r, &table, &mask, &blob);
      c->text.table.reset(); c->text.names.reset();
      HIPCHK(c, c->text.table.alloc(table.size()));
      HIPCHK(c, c->text.names.alloc(blob.size() + 4096 * 2 + 16));
      HIPCHK(c, hipMemcpy(c->text.table.get(), table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice));
      if (!blob.empty()) HIPCHK(c, hipMemcpy(c->text.names.get(), blob.data(), blob.size(), hipMemcpyHostToDevice));
      c->text.mask = mask; c->text.blobLen = (unsigned)blob.size(); c->text.blob = key;
    }
  }
  gtxtext::TextTables tabs; tabs.table = c->text.table.get(); tabs.tableMask = c->text.mask; tabs.names = c->text.names.get(); tabs.prevOff = 0; tabs.prevLen = 0;
  if (r->have_prev && r->prev_chrom) {
    const size_t len = strlen(r->prev_chrom);
    if (len > 0 && len < 4096) {                                       // the seam's name behind the names, one place per slot
      memcpy(t.seam.get(), r->prev_chrom, len);
      tabs.prevOff = c->text.blobLen + (unsigned)slot * 4096; tabs.prevLen = (unsigned)len;
      HIPCHK(c, hipMemcpyAsync(c->text.names.get() + tabs.prevOff, t.seam.get(), len, hipMemcpyHostToDevice, c->stream));
    }
  }
  // the text: page-locked memory is read where it is, anything else goes through a page-locked slot of the context
  const char *src = text;
  if (!is_pinned(text)) {
    if (bytes > t.pin.cap) HIPCHK(c, t.pin.alloc(bytes + (bytes >> 3)));
    parallel_copy(t.pin.get(), text, bytes, c->stage.copyThreads);
    src = t.pin.get();
  }
  HIPCHK(c, hipMemcpyAsync(t.text.get(), src, bytes, hipMemcpyHostToDevice, c->stage.copyStream));
  HIPCHK(c, hipEventRecord(t.evCopied, c->stage.copyStream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, t.evCopied, 0));
  HIPCHK(c, hipMemsetAsync(t.flag.get(), 0, sizeof(int), c->stream));
  if (format < 0) {                                                        // the newline index alone (gtx_blocks_text reads the text itself)
    HIPCHK(c, gtxtext::launch_newline_index(t.text.get(), bytes, t.seg.get(), t.nl.get(), (unsigned)nLines, c->stream));
    return GTX_OK;
  }
  grouped = grouped && r->strand_aware;
  if (grouped && (size_t)nLines > t.w2.cap) {
    t.tri2.reset(); t.blk.reset(); t.w2.reset();
    HIPCHK(c, t.tri2.alloc(3 * t.w.cap)); HIPCHK(c, t.blk.alloc(t.w.cap / 128 + 4)); HIPCHK(c, t.w2.alloc(t.w.cap));
  }
  gtxtext::TextDevice d; d.text = t.text.get(); d.segCount = t.seg.get(); d.nl = t.nl.get(); d.tri = t.tri.get(); d.w = t.w.get(); d.flag = t.flag.get();
  d.tri2 = grouped ? t.tri2.get() : nullptr; d.w2 = grouped ? t.w2.get() : nullptr; d.blkMinus = grouped ? t.blk.get() : nullptr;
  d.labelSum = labelSum; d.blockSum = t.sum.get();
  HIPCHK(c, gtxtext::launch_tokenize(d, tabs, *r, bytes, (unsigned)nLines, c->stream, scanRules, format));
  return GTX_OK;
}

static int add_text(gtx_ctx *c, TextMode mode, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, uint32_t flags, int *ticket)
{
  const bool coverage = mode == TEXT_COVER;
  const char *who = mode == TEXT_SCAN ? "gtx_scan_add_text" : coverage ? "gtx_coverage_add_text" : "gtx_count_add_text";
  if (mode == TEXT_SCAN ? !c->scan.cur.open : coverage ? !c->covOpen : !c->streamOpen) return fail(c, GTX_E_STATE, "gtx_*_add_text: no open count / coverage / scan call");
  if (mode == TEXT_SCAN && r && (r->max_label_value > 1) != c->scan.cur.weighted) return fail(c, GTX_E_ARG, "gtx_scan_add_text: the rules' label weights do not match gtx_scan_begin's");
  if (!text || !r || !ticket || nLines < 0 || bytes >= (1ull << 32) - 4096 || nLines >= (1ll << 31) || r->n_chrom < 0 || (r->n_chrom > 0 && !r->chrom_names))
    { c->err = std::string(who) + ": bad argument"; return GTX_E_ARG; }
  if ((flags & GTX_TEXT_SAM) && (flags & GTX_TEXT_GFF)) { c->err = std::string(who) + ": GTX_TEXT_SAM and GTX_TEXT_GFF exclude each other"; return GTX_E_ARG; }
  const int format = (flags & GTX_TEXT_SAM) ? 1 : (flags & GTX_TEXT_GFF) ? 2 : 0;   // (the format of the text, not a flag of the count: launch_tokenize's numbers)
  flags &= ~(GTX_TEXT_SAM | GTX_TEXT_GFF);
  TextSlot *tp = nullptr; bool empty = false;
  {
    int rc = text_stage(c, text, bytes, nLines, r, true, mode == TEXT_SCAN ? (c->scan.cur.a.sortedRule ? 2 : 1) : 0,
                        mode == TEXT_SCAN ? c->scan.cur.labelSum.get() : nullptr, format, &tp, ticket, &empty);
    if (rc || empty) return rc;
  }
  TextSlot &t = *tp;
  const int *triOut = r->strand_aware ? t.tri2.get() : t.tri.get();
  HIPCHK(c, hipMemcpyAsync(t.hostFlag.get(), t.flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(t.evParsed, c->stream));
  // ... and counted where the triples are
  const int *dW = r->max_label_value > 1 ? (r->strand_aware ? t.w2.get() : t.w.get()) : nullptr;
  const int64_t seen = c->streamSeen;
  int rc = GTX_OK;
  if (mode == TEXT_SCAN) {
    // (a block of a sorted stream is in order: the general kernels aggregate runs of equal micro-windows; any other block: the partition path)
    rc = scan_hist_any(c, triOut, dW, nLines, c->scan.cur.a, c->scan.cur.classLen.data(), (flags & GTX_READS_UNSORTED) != 0); if (rc) return rc;
    HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
    t.busy = true;
    return GTX_OK;
  }
  if (coverage) {
    if (flags & GTX_GAPS_FORMULA) { rc = merge_prepare(c, flags, 2); if (rc) return rc; }
    rc = cover_launch(c, triOut, dW, nLines, seen, flags, (flags & GTX_READS_UNSORTED) != 0 || !(flags & GTX_READS_SORTED)); if (rc) return rc;
  } else {
    rc = merge_prepare(c, flags, 0); if (rc) return rc;
    const bool streaming = (flags & (GTX_READS_SORTED | GTX_CHECK_SORTED)) != 0;
    if (!streaming) c->tileSumsValid = false;
    if (streaming) HIPCHK(c, gtx::launch_count(triOut, dW, nLines, count_args(c, c->ix.hist, flags & ~GTX_CHECK_SORTED, nLines, seen), true, c->stream));
    else { rc = launch_unsorted(c, triOut, dW, nLines, count_args(c, c->ix.hist, flags, nLines, seen)); if (rc) return rc; }
    rc = pairs_batch(c, triOut, dW, nLines); if (rc) return rc;
  }
  rc = merge_batch(c, triOut, dW, nLines); if (rc) return rc;
  HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
  t.busy = true;
  c->streamSeen += nLines;
  return GTX_OK;
}

// the sliding windows' view of a slot whose block gtx_windows_text has planned (gtx_windows.h)
static gtx::WindowsDevice windows_device(const TextSlot &t)
{
  const size_t nTiles = gtx::windows_tiles(t.wnLines);
  gtx::WindowsDevice d; d.text = t.text.get(); d.bytes = t.wnBytes; d.nl = t.nl.get(); d.nLines = t.wnLines; d.flag = t.flag.get();
  d.rec = t.wnRec.get(); d.tileWindows = t.wnTile.get(); d.tileBytes = t.wnTile.get() + nTiles; d.baseWindows = t.wnBase.get(); d.baseBytes = t.wnBase.get() + nTiles + 1;
  d.lineWin = t.wnLine.get(); d.lineByte = t.wnLine.get() + (size_t)t.wnLines + 1;
  return d;
}

// gtx_subset_result, gtx_rewrite_result, gtx_convert_result: the block's verdict and, of a block that stayed on the device, the
// hostTotal[0] bytes of its printed text copied to out, which holds `capacity` (SIZE_MAX: the entry point has no such argument), and
// its hostTotal[1] lines.  On the copy stream: the context's own may already hold the kernels of the block after this one
static int text_out_result(gtx_ctx *c, const char *name, TextPending family, int ticket, int *needs_host, char *out, size_t capacity, size_t *out_bytes, int64_t *n_lines)
{
  TextSlot *tp = nullptr;
  { int rc = textblock_result(c, name, family, ticket, needs_host, out_bytes != nullptr, &tp); if (rc) return rc; }
  TextSlot &t = *tp;
  *out_bytes = 0;
  if (n_lines) *n_lines = 0;
  if (*needs_host) return GTX_OK;
  const size_t n = (size_t)t.hostTotal.get()[0];
  if (n > 0 && (!out || n > capacity)) {
    const std::string who = std::string("gtx_") + name;
    c->err = capacity == SIZE_MAX ? who + "_result: bad argument" : who + "_result: out is missing or smaller than the block's text (" + who + "_max_bytes)";
    return GTX_E_ARG;
  }
  if (n > 0) { HIPCHK(c, hipMemcpyAsync(out, t.out.get(), n, hipMemcpyDeviceToHost, c->stage.copyStream)); HIPCHK(c, hipStreamSynchronize(c->stage.copyStream)); }
  *out_bytes = n;
  if (n_lines) *n_lines = (int64_t)t.hostTotal.get()[1];
  return GTX_OK;
}

extern "C" {
int gtx_count_add_text(gtx_ctx *c, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket)
{ return c ? add_text(c, TEXT_COUNT, text, bytes, n_lines, rules, flags, ticket) : GTX_E_ARG; }
int gtx_coverage_add_text(gtx_ctx *c, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket)
{ return c ? add_text(c, TEXT_COVER, text, bytes, n_lines, rules, flags, ticket) : GTX_E_ARG; }
int gtx_scan_add_text(gtx_ctx *c, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket)
{ return c ? add_text(c, TEXT_SCAN, text, bytes, n_lines, rules, flags, ticket) : GTX_E_ARG; }
int gtx_text_result(gtx_ctx *c, int ticket, int *needs_host)
{
  if (!c || !needs_host || (ticket & ~1)) return c ? fail(c, GTX_E_ARG, "gtx_text_result: bad argument") : GTX_E_ARG;
  TextSlot &t = c->text.slot[ticket];
  if (!t.evParsed) return fail(c, GTX_E_STATE, "gtx_text_result: no such block");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(t.evParsed));
  *needs_host = *t.hostFlag.get();
  return GTX_OK;
}

// text -> triples in line order -> hits -> verbatim check -> select, scan, gather; everything enqueued, the verdict and the totals
// on their way to the host behind it
int gtx_subset_text(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_text_rules *r, uint32_t flags, int *ticket)
{
  if (!c) return GTX_E_ARG;
  if (c->nRefs < 0) return fail(c, GTX_E_STATE, "gtx_subset_text: gtx_set_refs has not been called");
  if (!r || r->n_chrom < 0 || (r->n_chrom > 0 && !r->chrom_names) || (flags & (GTX_TEXT_SAM | GTX_TEXT_GFF)) || r->max_label_value > 1)
    return fail(c, GTX_E_ARG, "gtx_subset_text: bad argument");
  const int mode = join_mode(c, flags);
  { int rc = join_prepare(c); if (rc) return rc; }
  TextSlot *tp = nullptr; bool empty = false;
  { int rc = textblock_front(c, "subset", TEXT_SUBSET, text, bytes, nLines, ticket, r, 0, 0, &tp, &empty); if (rc || empty) return rc; }
  TextSlot &t = *tp;
  const size_t nTiles = gtxtext::subset_tiles((unsigned)nLines);
  if ((size_t)nLines > t.hits.cap) HIPCHK(c, t.hits.alloc(t.w.cap));
  if (2 * (nTiles + 1) > t.tile.cap) HIPCHK(c, t.tile.alloc(2 * (nTiles + 1) + (nTiles >> 2)));
  if (bytes > t.out.cap) HIPCHK(c, t.out.alloc(t.text.cap));
  const gtx::JoinQueries q{t.tri.get(), nullptr, nullptr, nLines};
  if (!c->join.info) HIPCHK(c, c->join.info.alloc(1));
  if ((size_t)nLines > c->join.off.cap) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, c->join.off.grow((size_t)nLines)); }   // (the block before may still be narrowing out of it)
  HIPCHK(c, gtx::launch_join_count(q, c->rx.pairAll.ix, ref_blocks(c), mode & ~gtx::JOIN_CHECK, c->join.off.get(), c->join.info.get(), c->stream));
  HIPCHK(c, gtx::launch_query_narrow(c->join.off.get(), nLines, t.hits.get(), c->stream));
  HIPCHK(c, gtxtext::launch_verbatim(t.text.get(), t.nl.get(), (unsigned)nLines, t.flag.get(), c->stream));
  const gtxtext::SubsetDevice d{t.text.get(), t.nl.get(), (unsigned)nLines, t.hits.get(), (flags & GTX_SUBSET_INVERT) ? 1 : 0, t.flag.get(), t.tile.get(), t.out.get()};
  HIPCHK(c, gtxtext::launch_subset_gather(d, c->stream));
  HIPCHK(c, hipMemcpyAsync(t.hostFlag.get(), t.flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&t.hostTotal.get()[0], t.tile.get() + nTiles, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&t.hostTotal.get()[1], t.tile.get() + 2 * nTiles + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(t.evParsed, c->stream));
  HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
  t.busy = true;
  return GTX_OK;
}

int gtx_subset_result(gtx_ctx *c, int ticket, int *needs_host, char *out, size_t *out_bytes, int64_t *n_selected)
{
  if (!c) return GTX_E_ARG;
  return text_out_result(c, "subset", TEXT_SUBSET, ticket, needs_host, out, SIZE_MAX, out_bytes, n_selected);
}

// text -> triples in line order (the tokenizer's plain case, the class of every line) -> plan, two prefixes, emit (gtx_rewrite.h);
// everything enqueued, the verdict and the totals on their way to the host behind it
int gtx_rewrite_text(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_rewrite_op *op, int *ticket)
{
  if (!c) return GTX_E_ARG;
  const int64_t kMaxAmount = 1ll << 62;                                    // columns of 10 digits stay far inside 64 bits with it
  if (!op || op->kind < GTX_REWRITE_SHIFT || op->kind > GTX_REWRITE_BOUNDS || op->a > kMaxAmount || op->a < -kMaxAmount || op->b > kMaxAmount || op->b < -kMaxAmount ||
      (op->kind == GTX_REWRITE_POS && (op->pos_op < GTX_REWRITE_POS_1 || op->pos_op > GTX_REWRITE_POS_C)) ||
      (op->kind == GTX_REWRITE_BOUNDS && (op->n_chrom < 0 || (op->n_chrom > 0 && (!op->chrom_names || !op->chrom_len)))))
    return fail(c, GTX_E_ARG, "gtx_rewrite_text: bad argument");
  const bool bounds = op->kind == GTX_REWRITE_BOUNDS;
  gtx_text_rules r; memset(&r, 0, sizeof r);                               // (bounds: the tokenizer's classes are the names' places)
  r.chrom_names = bounds ? op->chrom_names : nullptr; r.n_chrom = bounds ? op->n_chrom : 0; r.max_label_value = 1;
  TextSlot *tp = nullptr; bool empty = false;
  // (the sorted scanner's rules: nothing about the interval is checked, and without sorted_rules nothing about the order)
  { int rc = textblock_front(c, "rewrite", TEXT_REWRITE, text, bytes, nLines, ticket, &r, 2, 0, &tp, &empty); if (rc || empty) return rc; }
  TextSlot &t = *tp;
  if (bounds) {                                                            // the lengths per class: uploaded when they change
    std::vector<long long> len(op->chrom_len, op->chrom_len + op->n_chrom);
    if (len != c->text.h_chromLen || !c->text.chromLen) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, c->text.chromLen.alloc(len.size() + 1));
      if (!len.empty()) HIPCHK(c, hipMemcpy(c->text.chromLen.get(), len.data(), sizeof(long long) * len.size(), hipMemcpyHostToDevice));
      c->text.h_chromLen = len;
    }
  }
  const size_t nTiles = gtx::rewrite_tiles((unsigned)nLines), need = gtx_rewrite_max_bytes(bytes, nLines) + 32;
  if ((size_t)nLines > t.rwRec.cap) HIPCHK(c, t.rwRec.alloc(t.w.cap));
  if (2 * nTiles > t.rwTile.cap) { HIPCHK(c, t.rwTile.alloc(2 * nTiles + (nTiles >> 2))); HIPCHK(c, t.rwBase.alloc(2 * (nTiles + 1) + (nTiles >> 2))); }
  if (need > t.out.cap) HIPCHK(c, t.out.alloc(need + (need >> 3)));
  gtx::RewriteOp k; k.kind = op->kind; k.posOp = op->pos_op; k.a = op->a; k.b = op->b; k.chromLen = bounds ? c->text.chromLen.get() : nullptr; k.nChrom = bounds ? op->n_chrom : 0;
  gtx::RewriteDevice d; d.text = t.text.get(); d.bytes = bytes; d.nl = t.nl.get(); d.nLines = (unsigned)nLines; d.tri = t.tri.get(); d.flag = t.flag.get();
  d.rec = t.rwRec.get(); d.tileBytes = t.rwTile.get(); d.tileLines = t.rwTile.get() + nTiles; d.baseBytes = t.rwBase.get(); d.baseLines = t.rwBase.get() + nTiles + 1;
  d.out = t.out.get();
  prof_begin(c);                                                           // (gtx_profile_*: the plan, prefix and emit launches alone, on the text where it is)
  HIPCHK(c, prof_mark(c, 1, c->stream));
  HIPCHK(c, gtx::launch_rewrite(d, k, c->stream));
  return textblock_tail(c, t, d.baseBytes + nTiles, d.baseLines + nTiles);
}

int gtx_rewrite_result(gtx_ctx *c, int ticket, int *needs_host, char *out, size_t capacity, size_t *out_bytes, int64_t *n_printed)
{
  if (!c) return GTX_E_ARG;
  return text_out_result(c, "rewrite", TEXT_REWRITE, ticket, needs_host, out, capacity, out_bytes, n_printed);
}

size_t gtx_rewrite_max_bytes(size_t bytes, int64_t n_lines) { return bytes + (size_t)gtx::kRewriteGrow * (size_t)(n_lines > 0 ? n_lines : 0); }

int gtx_rewrite_limits(int32_t *tile, int32_t *stage)
{
  if (tile) *tile = gtx::kRewriteTile;
  if (stage) *stage = gtx::kRewriteStage;
  return GTX_OK;
}

// text of any of the three formats -> the tokenizer's verdict (its plain case; no names, so its triples are not read) -> plan, prefix,
// emit (gtx_convert.h); everything enqueued, the verdict and the total on their way to the host behind it
int gtx_convert_text(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_convert_op *op, uint32_t flags, int *ticket)
{
  if (!c) return GTX_E_ARG;
  const bool sam = (flags & GTX_TEXT_SAM) != 0, gff = (flags & GTX_TEXT_GFF) != 0;
  const size_t colorLen = op && op->color ? strlen(op->color) : 0;
  if (!op || (flags & ~(GTX_TEXT_SAM | GTX_TEXT_GFF)) || (sam && gff) || (op->to != GTX_CONVERT_BED && op->to != GTX_CONVERT_REG) ||
      (op->to == GTX_CONVERT_BED && !sam && !gff) || colorLen > (size_t)gtx::kConvertMaxColor)
    return fail(c, GTX_E_ARG, "gtx_convert_text: bad argument");
  const int format = sam ? 1 : gff ? 2 : 0;                                // (launch_tokenize's numbers)
  TextSlot *tp = nullptr; bool empty = false;
  // (the sorted scanner's rules, as for the rewrite: nothing about the interval is checked, and nothing about the order)
  { int rc = textblock_front(c, "convert", TEXT_CONVERT, text, bytes, nLines, ticket, nullptr, 2, format, &tp, &empty); if (rc || empty) return rc; }
  TextSlot &t = *tp;
  const size_t nTiles = gtx::convert_tiles((unsigned)nLines), need = gtx_convert_max_bytes(bytes, nLines, op) + 32;
  if ((size_t)nLines > t.cvRec.cap) HIPCHK(c, t.cvRec.alloc(t.w.cap));
  if (nTiles > t.cvTile.cap) { HIPCHK(c, t.cvTile.alloc(nTiles + (nTiles >> 2))); HIPCHK(c, t.cvBase.alloc(nTiles + 1 + (nTiles >> 2))); }
  if (need > t.out.cap) HIPCHK(c, t.out.alloc(need + (need >> 3)));
  gtx::ConvertOp k; memset(&k, 0, sizeof k);
  k.to = op->to == GTX_CONVERT_REG ? gtx::kConvertReg : gtx::kConvertBed; k.ucsc = op->ucsc_names ? 1 : 0;
  k.colorLen = k.to == gtx::kConvertBed ? (int)colorLen : 0;              // (reg's -c prints a single-interval region as it stands)
  if (k.colorLen) memcpy(k.color, op->color, colorLen);
  gtx::ConvertDevice d; d.text = t.text.get(); d.bytes = bytes; d.nl = t.nl.get(); d.nLines = (unsigned)nLines; d.format = format; d.flag = t.flag.get();
  d.rec = t.cvRec.get(); d.tileBytes = t.cvTile.get(); d.baseBytes = t.cvBase.get(); d.out = t.out.get();
  t.hostTotal.get()[1] = (unsigned long long)nLines;                       // (every line of a plain block is printed)
  prof_begin(c);                                                           // (gtx_profile_*: the plan, prefix and emit launches alone, on the text where it is)
  HIPCHK(c, prof_mark(c, 1, c->stream));
  HIPCHK(c, gtx::launch_convert(d, k, c->stream));
  return textblock_tail(c, t, d.baseBytes + nTiles, nullptr);
}

int gtx_convert_result(gtx_ctx *c, int ticket, int *needs_host, char *out, size_t capacity, size_t *out_bytes, int64_t *n_printed)
{
  if (!c) return GTX_E_ARG;
  return text_out_result(c, "convert", TEXT_CONVERT, ticket, needs_host, out, capacity, out_bytes, n_printed);
}

size_t gtx_convert_max_bytes(size_t bytes, int64_t n_lines, const gtx_convert_op *op)
{
  const size_t colorLen = op && op->color ? strlen(op->color) : 0;
  const size_t grow = (size_t)gtx::kConvertGrow + (colorLen ? (size_t)gtx::kConvertGrowColor + colorLen : 0);
  return bytes + grow * (size_t)(n_lines > 0 ? n_lines : 0);
}

int gtx_convert_limits(int32_t *tile, int32_t *stage, int32_t *max_color)
{
  if (tile) *tile = gtx::kConvertTile;
  if (stage) *stage = gtx::kConvertStage;
  if (max_color) *max_color = gtx::kConvertMaxColor;
  return GTX_OK;
}

// text -> triples in line order (the tokenizer's plain case) -> plan, two 64-bit prefixes, the lines' bases (gtx_windows.h);
// everything enqueued, the verdict and the totals on their way to the host behind it.  Nothing is rendered before gtx_windows_result
int gtx_windows_text(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_windows_op *op, int *ticket)
{
  if (!c) return GTX_E_ARG;
  if (!op || op->win_size < 1 || op->win_size > (1ll << 31) || op->win_step < 1 || op->win_step > (1ll << 31))
    return fail(c, GTX_E_ARG, "gtx_windows_text: bad argument");
  TextSlot *tp = nullptr; bool empty = false;
  // (the sorted scanner's rules, as for the rewrite: nothing about the interval is checked, and nothing about the order)
  { int rc = textblock_front(c, "windows", TEXT_WINDOWS, text, bytes, nLines, ticket, nullptr, 2, 0, &tp, &empty); if (rc) return rc; }
  TextSlot &t = *tp;
  t.wnSize = op->win_size; t.wnStep = op->win_step; t.wnSmall = op->small ? 1 : 0; t.wnBytes = bytes; t.wnLines = (unsigned)nLines;
  if (empty) { t.wnLines = 0; return GTX_OK; }
  const size_t nTiles = gtx::windows_tiles((unsigned)nLines);
  if ((size_t)nLines > t.wnRec.cap) { HIPCHK(c, t.wnRec.alloc(t.w.cap)); HIPCHK(c, t.wnLine.alloc(2 * (t.w.cap + 1))); }
  if (2 * nTiles > t.wnTile.cap) { HIPCHK(c, t.wnTile.alloc(2 * nTiles + (nTiles >> 2))); HIPCHK(c, t.wnBase.alloc(2 * (nTiles + 1) + (nTiles >> 2))); }
  const gtx::WindowsDevice d = windows_device(t);
  const gtx::WindowsOp k{t.wnSize, t.wnStep, t.wnSmall};
  prof_begin(c);                                                           // (gtx_profile_*: the plan, prefix and base launches alone, on the text where it is)
  HIPCHK(c, prof_mark(c, 1, c->stream));
  HIPCHK(c, gtx::launch_windows_plan(d, k, c->stream));
  return textblock_tail(c, t, d.baseWindows + nTiles, d.baseBytes + nTiles);
}

// The block's windows in ranges of whole output tiles through two device and two page-locked buffers, as gtx_window_lines streams
// its lines: range r + 1 is enqueued before the sink is given range r - 1, behind the copy of r - 1 out of the device buffer it
// writes.  A range's place in the output is the sum of the ranges in front, known when it is enqueued.
int gtx_windows_result(gtx_ctx *c, int ticket, int *needs_host, gtx_lines_sink sink, void *user, int64_t *n_windows, int64_t *n_bytes)
{
  if (!c) return GTX_E_ARG;
  TextSlot *tp = nullptr;
  { int rc = textblock_result(c, "windows", TEXT_WINDOWS, ticket, needs_host, true, &tp); if (rc) return rc; }
  TextSlot &t = *tp;
  TextState &s = c->text;
  if (n_windows) *n_windows = 0;
  if (n_bytes) *n_bytes = 0;
  if (*needs_host) return GTX_OK;
  const int64_t total = (int64_t)t.hostTotal.get()[0], totalBytes = (int64_t)t.hostTotal.get()[1];
  if (total == 0) return GTX_OK;
  if (!sink) return fail(c, GTX_E_ARG, "gtx_windows_result: a sink is required");
  const int64_t W = gtx::kWindowsOutTile, allTiles = (total + W - 1) / W;
  const int64_t per = std::min(allTiles, std::max<int64_t>(1, c->lines.chunkBytes / gtx::kWindowsRunBytes));   // output tiles per range
  const size_t room = (size_t)per * gtx::kWindowsRunBytes + 32;
  if (room > s.wnOut[0].cap || room > s.wnPin[0].cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipStreamSynchronize(c->stage.copyStream));
    for (int k = 0; k < 2; k++) { HIPCHK(c, s.wnOut[k].reserve(room)); HIPCHK(c, s.wnPin[k].reserve(room)); }
  }
  for (int k = 0; k < 2; k++) if (!s.wnCopied[k]) HIPCHK(c, hipEventCreateWithFlags(&s.wnCopied[k], hipEventDisableTiming));
  if (!s.wnRange) { HIPCHK(c, s.wnRange.alloc(2)); HIPCHK(c, s.wnHostRange.alloc(2)); }
  const gtx::WindowsDevice d = windows_device(t);
  const gtx::WindowsOp op{t.wnSize, t.wnStep, t.wnSmall};
  const int64_t ranges = (allTiles + per - 1) / per;
  int64_t got[2] = {0, 0}, done = 0;                                       // the bytes of the ranges in the two page-locked buffers; of all ranges finished
  auto enqueue = [&](int64_t r, int64_t base) -> int {                     // (gtx_profile_*: a range's emit launch alone is one profiled call)
    const int k = (int)(r & 1);
    const gtx::WindowsRange rg{r * per * W, std::min(per, allTiles - r * per), base, total, s.wnOut[k].get(), s.wnRange.get() + k};
    prof_begin(c);
    HIPCHK(c, prof_mark(c, 1, c->stream));
    HIPCHK(c, gtx::launch_windows_emit(d, op, rg, c->stream));
    HIPCHK(c, prof_mark(c, 2, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.wnHostRange.get() + k, s.wnRange.get() + k, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, prof_end(c, c->stream));
    return GTX_OK;
  };
  auto sink_range = [&](int64_t r) -> int {
    const int k = (int)(r & 1);
    HIPCHK(c, hipEventSynchronize(s.wnCopied[k]));
    if (got[k] > 0 && sink(user, s.wnPin[k].get(), (size_t)got[k]) != 0) {
      (void)hipStreamSynchronize(c->stream); (void)hipStreamSynchronize(c->stage.copyStream);
      c->err = "gtx_windows_result: the sink refused the text"; return GTX_E_SINK;
    }
    return GTX_OK;
  };
  int rc = enqueue(0, 0); if (rc) return rc;
  for (int64_t r = 0; r < ranges; r++) {
    const int k = (int)(r & 1);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    got[k] = (int64_t)s.wnHostRange.get()[k];
    if (got[k] < 0 || (size_t)got[k] + 32 > room) { (void)hipStreamSynchronize(c->stage.copyStream); return fail(c, GTX_E_STATE, "gtx_windows_result: a range outside its bound"); }
    HIPCHK(c, hipMemcpyAsync(s.wnPin[k].get(), s.wnOut[k].get(), (size_t)got[k], hipMemcpyDeviceToHost, c->stage.copyStream));
    HIPCHK(c, hipEventRecord(s.wnCopied[k], c->stage.copyStream));
    done += got[k];
    if (r + 1 < ranges) {
      if (r >= 1) HIPCHK(c, hipStreamWaitEvent(c->stream, s.wnCopied[k ^ 1], 0));   // the copy of r - 1 out of the buffer r + 1 is rendered into
      rc = enqueue(r + 1, done); if (rc) return rc;
    }
    if (r >= 1) { rc = sink_range(r - 1); if (rc) return rc; }
  }
  rc = sink_range(ranges - 1); if (rc) return rc;
  if (done != totalBytes) return fail(c, GTX_E_STATE, "gtx_windows_result: the ranges' bytes differ from the plan's");
  if (n_windows) *n_windows = total;
  if (n_bytes) *n_bytes = done;
  return GTX_OK;
}

int gtx_windows_limits(int32_t *line_tile, int32_t *out_tile, int32_t *max_fixed)
{
  if (line_tile) *line_tile = gtx::kWindowsLineTile;
  if (out_tile) *out_tile = gtx::kWindowsOutTile;
  if (max_fixed) *max_fixed = gtx::kWindowsMaxFixed;
  return GTX_OK;
}
}
