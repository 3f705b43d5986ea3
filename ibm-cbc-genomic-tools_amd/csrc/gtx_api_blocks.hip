// gtx_api_blocks.hip -- the C ABI's block operations on region text (gtx_blocks_*): split, connect, select, diff, n and strand of
// BED lines, the 12-column ones included.  Host code only (the kernels: gtx_blocks.hip, and gtx_text.hip for the newline index); the
// text reaches the device through text_stage of gtx_api_text.hip behind the handshake of gtx_api_textblock.h, the context is in gtx_ctx.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include "gtx.h"
#include "gtx_blocks.h"
#include "gtx_ctx.h"
#include "gtx_api_textblock.h"

// the passes' view of a slot whose block gtx_blocks_text has planned (gtx_blocks.h)
static gtx::BlocksDevice blocks_device(const TextSlot &t)
{
  const size_t nTiles = gtx::blocks_tiles(t.blLines), nSeg = (t.blBytes + 1023) / 1024;
  gtx::BlocksDevice d; d.text = t.text.get(); d.bytes = t.blBytes; d.nl = t.nl.get(); d.nlTotal = t.seg.get() + nSeg; d.nLines = t.blLines; d.flag = t.flag.get();
  d.rec = t.blRec.get(); d.tileBytes = t.blTile.get(); d.tileCount = t.blTile.get() + nTiles; d.baseBytes = t.blBase.get(); d.baseCount = t.blBase.get() + nTiles + 1;
  d.lineOut = t.blLineOut.get(); d.lineByte = t.blLineByte.get();
  return d;
}

extern "C" {
// text -> newline index -> plan, two prefixes, split's bases of the lines (gtx_blocks.h); everything enqueued, the verdict and the
// totals on their way to the host behind it.  Nothing is rendered before gtx_blocks_result
int gtx_blocks_text(gtx_ctx *c, const char *text, size_t bytes, int64_t nLines, const gtx_blocks_op *op, int *ticket)
{
  if (!c) return GTX_E_ARG;
  if (!op || op->kind < GTX_BLOCKS_SPLIT || op->kind > GTX_BLOCKS_STRAND || (op->select & ~(GTX_BLOCKS_FIRST | GTX_BLOCKS_LAST | GTX_BLOCKS_5P | GTX_BLOCKS_3P)) ||
      op->strand_op < GTX_BLOCKS_STRAND_PLUS || op->strand_op > GTX_BLOCKS_STRAND_REVERSE)
    return fail(c, GTX_E_ARG, "gtx_blocks_text: bad argument");
  TextSlot *tp = nullptr; bool empty = false;
  // (format -1: the newline index alone, the passes read the text themselves)
  { int rc = textblock_front(c, "blocks", TEXT_BLOCKS, text, bytes, nLines, ticket, nullptr, 0, -1, &tp, &empty); if (rc) return rc; }
  TextSlot &t = *tp;
  t.blKind = op->kind; t.blSelect = op->select; t.blStrand = op->strand_op; t.blBytes = bytes; t.blLines = (unsigned)nLines;
  if (empty) { t.blLines = 0; return GTX_OK; }
  const size_t nTiles = gtx::blocks_tiles((unsigned)nLines);
  if ((size_t)nLines > t.blRec.cap) HIPCHK(c, t.blRec.alloc(t.w.cap));
  if (op->kind == GTX_BLOCKS_SPLIT && (size_t)nLines + 1 > t.blLineOut.cap) { HIPCHK(c, t.blLineOut.alloc(t.w.cap + 1)); HIPCHK(c, t.blLineByte.alloc(t.w.cap + 1)); }
  if (2 * nTiles > t.blTile.cap) { HIPCHK(c, t.blTile.alloc(2 * nTiles + (nTiles >> 2))); HIPCHK(c, t.blBase.alloc(2 * (nTiles + 1) + (nTiles >> 2))); }
  const gtx::BlocksDevice d = blocks_device(t);
  const gtx::BlocksOp k{op->kind, op->select, op->strand_op};
  prof_begin(c);                                                           // (gtx_profile_*: the plan, prefix and base launches alone, on the text where it is)
  HIPCHK(c, prof_mark(c, 1, c->stream));
  HIPCHK(c, gtx::launch_blocks_plan(d, k, c->stream));
  return textblock_tail(c, t, d.baseBytes + nTiles, d.baseCount + nTiles);
}

// The block's printed text: rendered into one device buffer, copied into one page-locked buffer, handed to the sink in pieces that
// end at a line's end.  The emit launch follows whatever the stream already holds of the block behind this one.
int gtx_blocks_result(gtx_ctx *c, int ticket, int *needs_host, gtx_lines_sink sink, void *user, int64_t *n_printed, int64_t *n_bytes)
{
  if (!c) return GTX_E_ARG;
  TextSlot *tp = nullptr;
  { int rc = textblock_result(c, "blocks", TEXT_BLOCKS, ticket, needs_host, true, &tp); if (rc) return rc; }
  TextSlot &t = *tp;
  TextState &s = c->text;
  if (n_printed) *n_printed = 0;
  if (n_bytes) *n_bytes = 0;
  if (*needs_host || t.blLines == 0) return GTX_OK;
  const size_t total = (size_t)t.hostTotal.get()[0];
  const int64_t lines = (int64_t)t.hostTotal.get()[1];
  if (total == 0) return GTX_OK;
  if (!sink) return fail(c, GTX_E_ARG, "gtx_blocks_result: a sink is required");
  const size_t room = total + 32;
  if (room > s.blOut.cap || room > s.blPin.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, s.blOut.reserve(room, room + (room >> 3))); HIPCHK(c, s.blPin.reserve(room, room + (room >> 3)));
  }
  const gtx::BlocksDevice d = blocks_device(t);
  const gtx::BlocksOp k{t.blKind, t.blSelect, t.blStrand};
  prof_begin(c);                                                           // (gtx_profile_*: the emit launch alone is one profiled call)
  HIPCHK(c, prof_mark(c, 1, c->stream));
  HIPCHK(c, gtx::launch_blocks_emit(d, k, lines, s.blOut.get(), c->stream));
  HIPCHK(c, prof_mark(c, 2, c->stream));
  HIPCHK(c, hipMemcpyAsync(s.blPin.get(), s.blOut.get(), total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, prof_end(c, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const char *p = s.blPin.get(), *end = p + total;
  const size_t chunk = std::max<size_t>((size_t)c->lines.chunkBytes, 1);
  while (p < end) {
    size_t n = std::min<size_t>(chunk, (size_t)(end - p));
    if (p + n < end) {                                                     // back to the last line's end inside the piece; a line longer than a piece goes whole
      const void *nl = memrchr(p, '\n', n);
      if (nl) n = (size_t)((const char *)nl - p) + 1;
      else { const void *fw = memchr(p + n, '\n', (size_t)(end - p) - n); n = fw ? (size_t)((const char *)fw - p) + 1 : (size_t)(end - p); }
    }
    if (sink(user, p, n) != 0) { c->err = "gtx_blocks_result: the sink refused the text"; return GTX_E_SINK; }
    p += n;
  }
  if (n_printed) *n_printed = lines;
  if (n_bytes) *n_bytes = (int64_t)total;
  return GTX_OK;
}

size_t gtx_blocks_max_bytes(size_t bytes, int64_t n_lines, const gtx_blocks_op *op)
{
  if (!op || op->kind == GTX_BLOCKS_SPLIT) return 0;
  return 7 * bytes + 96 * (size_t)(n_lines > 0 ? n_lines : 0);
}

int gtx_blocks_limits(int32_t *tile, int32_t *stage, int32_t *max_blocks)
{
  if (tile) *tile = gtx::kBlocksTile;
  if (stage) *stage = gtx::kBlocksStage;
  if (max_blocks) *max_blocks = gtx::kBlocksMax;
  return GTX_OK;
}
}
