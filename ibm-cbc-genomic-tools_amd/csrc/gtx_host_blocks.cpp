// gtx_host_blocks.cpp -- the per-region operations of genomic_regions that look inside a region's intervals, on a streamed BED set:
// split, connect, select, diff, n and strand (GenomicRegionSet::RunSplit, RunConnect, RunSelect, RunDiff, RunSize, RunModifyStrand).
// See genomic_intervals.h; the host loop, Print and UpdateThick are gtx_host_regionops.cpp's, through gtx_host.h.
#include "gtx_host.h"

#include <algorithm>

using namespace gtx_host;

namespace {

struct BlocksSpec { int kind; bool first, last, from5p, from3p; std::string strand_op; };

// one region through the operation and out, as GenomicRegionBED's members have it
void RenderBlocks(std::string &out, const BlocksSpec &op, GenomicRegion *r, const std::string &raw)
{
  PairQuery q = PairQuery::From(r, raw);
  std::vector<long int> &iv = q.iv;
  const size_t n = iv.size() / 2;
  char num[96];
  switch (op.kind) {
    case GTX_BLOCKS_SPLIT:                                        // RunSplit :2502-2505 over PrintModified :2310-2314
      for (size_t k = 0; k < n; k++) {
        out += q.chrom;
        out.append(num, (size_t)snprintf(num, sizeof num, "\t%ld\t%ld\t", iv[2 * k] - 1, iv[2 * k + 1]));
        out += q.label;
        out.append(num, (size_t)snprintf(num, sizeof num, "\t%ld\t%c\n", q.score, q.strand));
        WriteOut(out, 1u << 22);
      }
      break;
    case GTX_BLOCKS_SIZE: {                                       // RunSize :1451-1454 over GetSize :1047-1055, :488-491
      unsigned long size = 0;
      for (size_t k = 0; k < n; k++) if (iv[2 * k] <= iv[2 * k + 1]) size += (unsigned long)(iv[2 * k + 1] - iv[2 * k] + 1);
      out += q.label;
      out.append(num, (size_t)snprintf(num, sizeof num, "\t%lu\n", size));
      break;
    }
    case GTX_BLOCKS_CONNECT:                                      // Connect :1319-1339
      if (n > 1) {
        long int start = iv[0], stop = iv[1];
        for (size_t k = 1; k < n; k++) { start = std::min(start, iv[2 * k]); stop = std::max(stop, iv[2 * k + 1]); }
        iv.assign({start, stop});
      }
      break;
    case GTX_BLOCKS_SELECT: {                                     // Select :1493-1521 (Sort is a no-op for BED, :2493-2496)
      if (n == 0) break;
      const bool pos_first = op.first || (op.from5p && q.strand == '+') || (op.from3p && q.strand == '-');
      const bool pos_last = op.last || (op.from5p && q.strand == '-') || (op.from3p && q.strand == '+');
      if (!pos_first && !pos_last) iv.clear();
      else if (n == 1) break;
      else if (pos_first && pos_last) { if (n > 2) iv.assign({iv[0], iv[1], iv[2 * n - 2], iv[2 * n - 1]}); }
      else if (pos_first) iv.resize(2);
      else iv.assign({iv[2 * n - 2], iv[2 * n - 1]});
      break;
    }
    case GTX_BLOCKS_DIFF: {                                       // Diff :1345-1361
      if (n <= 1) { iv.clear(); break; }
      if (!r->IsCompatibleSortedAndNonoverlapping()) r->PrintError("region intervals must be compatible, sorted and non-overlapping for this operation!");
      std::vector<long int> gaps;
      for (size_t k = 1; k < n; k++)
        if (iv[2 * k] - 1 >= iv[2 * k - 1] + 1) { gaps.push_back(iv[2 * k - 1] + 1); gaps.push_back(iv[2 * k] - 1); }
      iv.swap(gaps);
      break;
    }
    default:                                                      // ModifyStrand :1607-1620: any other word changes nothing
      if (op.strand_op == "r") q.strand = q.strand == '+' ? '-' : q.strand == '-' ? '+' : q.strand;
      else if (op.strand_op == "+") q.strand = '+';
      else if (op.strand_op == "-") q.strand = '-';
  }
  if (op.kind != GTX_BLOCKS_SPLIT && op.kind != GTX_BLOCKS_SIZE && !iv.empty()) {
    if (op.kind != GTX_BLOCKS_STRAND) UpdateThick(q);
    Print(out, q, r->n_line);
  }
  WriteOut(out, 1u << 22);
}

// the set's text through gtx_blocks_text; gtx_blocks_result streams a block's printed lines to stdout (DeviceTextLoop)
void BlocksTextLoop(GenomicRegionSet *set, const gtx_blocks_op &dev, const Renderer &render)
{
  LineFamily f{"[gtx blocks] blocks rendered on the device", false, false, {}, nullptr, nullptr, NULL};
  f.add = [&](gtx_ctx *ctx, const TextPump::Block &b) {
    int ticket = -1;
    DieGtx(ctx, gtx_blocks_text(ctx, b.text, b.bytes, b.n_lines, &dev, &ticket));
    return ticket;
  };
  f.result = [](gtx_ctx *ctx, int ticket, const TextPump::Block &) {
    int redo = 0;
    DieGtx(ctx, gtx_blocks_result(ctx, ticket, &redo, WriteSink, stdout, NULL, NULL));
    return redo != 0;
  };
  DeviceTextLoop(set, f, render);
}

void RunBlocks(GenomicRegionSet *set, const BlocksSpec &op)
{
  if (set->n_regions == 0) return;
  if (set->format != "BED") set->PrintError("unsupported input format!\n");
  if (set->load_in_memory) set->PrintError("the block operations stream their input on the MI355X path: open the set with load_in_memory = false!");
  // GTX_TEXT_ON_DEVICE=0: the host loop and nothing else.  Otherwise the device is looked for whatever the input's size: without
  // one the run ends with the library's error, as every other operation's does
  bool device = !TextPolicy().never && OneGpuWithPool();   // whatever the input's size
  gtx_blocks_op dev; memset(&dev, 0, sizeof dev);
  dev.kind = op.kind;
  dev.select = (op.first ? GTX_BLOCKS_FIRST : 0) | (op.last ? GTX_BLOCKS_LAST : 0) | (op.from5p ? GTX_BLOCKS_5P : 0) | (op.from3p ? GTX_BLOCKS_3P : 0);
  if (op.strand_op == "-") dev.strand_op = GTX_BLOCKS_STRAND_MINUS;
  else if (op.strand_op == "r") dev.strand_op = GTX_BLOCKS_STRAND_REVERSE;
  else if (op.kind == GTX_BLOCKS_STRAND && op.strand_op != "+") device = false;   // a word that changes nothing: the loop prints every region as it is
  const Renderer render = [&op](std::string &out, GenomicRegion *r, const std::string &raw) { RenderBlocks(out, op, r, raw); };
  if (device) BlocksTextLoop(set, dev, render);
  else HostLoop(set, render);
}

}  // namespace

void GenomicRegionSet::RunSplit(bool) { RunBlocks(this, BlocksSpec{GTX_BLOCKS_SPLIT, false, false, false, false, ""}); }   // (by_chrom_and_strand: REG only, :2502)
void GenomicRegionSet::RunConnect() { RunBlocks(this, BlocksSpec{GTX_BLOCKS_CONNECT, false, false, false, false, ""}); }
void GenomicRegionSet::RunSelect(bool first, bool last, bool from5p, bool from3p) { RunBlocks(this, BlocksSpec{GTX_BLOCKS_SELECT, first, last, from5p, from3p, ""}); }
void GenomicRegionSet::RunDiff() { RunBlocks(this, BlocksSpec{GTX_BLOCKS_DIFF, false, false, false, false, ""}); }
void GenomicRegionSet::RunSize() { RunBlocks(this, BlocksSpec{GTX_BLOCKS_SIZE, false, false, false, false, ""}); }
void GenomicRegionSet::RunModifyStrand(const char *strand_op) { RunBlocks(this, BlocksSpec{GTX_BLOCKS_STRAND, false, false, false, false, strand_op ? strand_op : "+"}); }
