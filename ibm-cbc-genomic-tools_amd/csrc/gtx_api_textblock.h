// gtx_api_textblock.h -- the handshake of the entry points that take a block of text lines and hand text back under a ticket:
// gtx_subset_*, gtx_rewrite_*, gtx_windows_*, gtx_convert_* (gtx_api_text.hip) and gtx_blocks_* (gtx_api_blocks.hip).  A slot holds
// one block: TextSlot::pending says whose, from the family's _text call until its _result call.  `name` is the family's word in its
// entry points' names ("rewrite": gtx_rewrite_text, gtx_rewrite_result, gtx_rewrite_max_bytes), for the error texts.  Host code.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include "gtx.h"
#include "gtx_ctx.h"
#pragma GCC visibility push(hidden)

// The front of gtx_<name>_text, behind the checks of what is the family's own: the bounds every block has, the slot whose turn it is
// (refused while it holds a block of this family that has not been fetched; a block of another family is forgotten), the text staged
// and tokenised (text_stage; rules: the caller's, or none for no names and no label weights), the totals on the host zeroed, the
// slot marked.  *tp, *ticket, *empty as text_stage leaves them.
inline int textblock_front(gtx_ctx *c, const char *name, TextPending family, const char *text, size_t bytes, int64_t nLines, int *ticket,
                           const gtx_text_rules *rules, int scanRules, int format, TextSlot **tp, bool *empty)
{
  const std::string who = std::string("gtx_") + name;
  if (!text || !ticket || nLines < 0 || bytes >= (1ull << 32) - 4096 || nLines >= (1ll << 31)) { c->err = who + "_text: bad argument"; return GTX_E_ARG; }
  if (c->text.slot[c->text.seq & 1].pending == family)
    { c->err = who + "_text: the result of the block before last has not been fetched (" + who + "_result)"; return GTX_E_STATE; }
  gtx_text_rules plain; memset(&plain, 0, sizeof plain);
  plain.max_label_value = 1;
  { int rc = text_stage(c, text, bytes, nLines, rules ? rules : &plain, false, scanRules, nullptr, format, tp, ticket, empty); if (rc) return rc; }
  TextSlot &t = **tp;
  if (!t.hostTotal) HIPCHK(c, t.hostTotal.alloc(2));
  t.hostTotal.get()[0] = t.hostTotal.get()[1] = 0;
  t.pending = family;
  return GTX_OK;
}

// The tail of a profiled gtx_<name>_text, behind its launches: the verdict and up to two 64-bit totals (device addresses, or null)
// on their way to the host inside the profile's bracket, the slot's events, the slot busy.
inline int textblock_tail(gtx_ctx *c, TextSlot &t, const long long *total0, const long long *total1)
{
  HIPCHK(c, prof_mark(c, 2, c->stream));
  HIPCHK(c, hipMemcpyAsync(t.hostFlag.get(), t.flag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (total0) HIPCHK(c, hipMemcpyAsync(&t.hostTotal.get()[0], total0, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  if (total1) HIPCHK(c, hipMemcpyAsync(&t.hostTotal.get()[1], total1, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, prof_end(c, c->stream));
  HIPCHK(c, hipEventRecord(t.evParsed, c->stream));
  HIPCHK(c, hipEventRecord(t.evConsumed, c->stream));
  t.busy = true;
  return GTX_OK;
}

// The head of gtx_<name>_result: the ticket's slot, which must hold a block of this family (argsOk: the family's own pointers are
// there); waits for the block's verdict, forgets the block and hands out the verdict.
inline int textblock_result(gtx_ctx *c, const char *name, TextPending family, int ticket, int *needs_host, bool argsOk, TextSlot **tp)
{
  const std::string who = std::string("gtx_") + name;
  if (!needs_host || !argsOk || (ticket & ~1)) { c->err = who + "_result: bad argument"; return GTX_E_ARG; }
  TextSlot &t = c->text.slot[ticket];
  if (!t.evParsed || t.pending != family) { c->err = who + "_result: no such block"; return GTX_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(t.evParsed));
  t.pending = TEXT_NONE;
  *needs_host = *t.hostFlag.get();
  *tp = &t;
  return GTX_OK;
}
#pragma GCC visibility pop
