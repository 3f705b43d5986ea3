// gtx_host.h -- what the sources of the host class layer share: genomic_intervals.cpp (the region classes and sets) and one
// gtx_host_*.cpp per family of drivers (device start-up and hand-over, the reductions, the scanners, the join users, link and the
// neighbour passes).  Private to csrc: the CLIs and the callers under tests/tools see genomic_intervals.h only.  What a single source
// uses stays in that source.
#pragma once
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <functional>
#include <future>
#include <string>
#include <vector>

#include "genomic_intervals.h"
#include "gtx.h"
#include "gtx_bed.h"

namespace gtx_host {

using gtxhost::BedPacker;
using gtxhost::ChromTable;
using gtxhost::LineSource;
using gtxhost::PackedBatch;
using gtxhost::PackError;
using gtxhost::PackOptions;

// ---- genomic_intervals.cpp: region memory and the errors of a set's lines --------------------------------------------------
char *CopyString(const char *s);                                  // into region memory (GtxRegionAlloc)

// The threads that build an in-memory set (GenomicRegionSet::Init) must not exit() on a malformed line -- another thread may hold
// an earlier one: they note the error here and unwind; Init raises the one with the smallest line number, as the reference's
// line-by-line reader would have.  The drivers' query loops catch the errors of the class layer the same way.
struct LoadError { bool set = false; long int line = 0; std::string msg; bool with_prefix = true; };
struct LoadAbort {};
extern thread_local LoadError *tls_load_error;
void DieLine(long int n_line, const std::string &msg);
void DiePack(const PackError &e);

// a strand-aware run over the regions of an in-memory GFF set: a strand byte other than '+' or '-' is an input error at its line
// (the engine has two strand classes per chromosome; see gtxhost::GffStrandMessage).  Call before anything renumbers n_line.
void CheckGffStrands(GenomicRegionSet *set);

inline bool FitsPacked(long int v) { return v < INT_MAX - 1 && v > INT_MIN + 1; }   // the packed 32-bit representation takes it

// ---- gtx_host_join.cpp: a BED line printed again, for the drivers that print query lines -------------------------------------
// what GenomicRegionBED::Print (genomic_intervals.cpp:2188-2220) needs of a query, kept until it is printed
struct PairQuery {
  std::string chrom, label, rgb;
  char strand;
  long int n_tokens, score, thick_start, thick_end;
  std::vector<long int> iv;                                        // start, stop of every interval
  static PairQuery From(GenomicRegion *q, const std::string &current_line);   // of the BED region a loop hands out and its raw line
};
// GenomicRegionBED::Print of a region with these intervals and this label
void PrintBed(std::string &out, const PairQuery &q, const std::vector<long int> &iv, const std::string &label, long int score,
              long int thick_start, long int thick_end);
void WriteOut(std::string &out, size_t above = 0);                // the text so far to stdout once it is longer than `above`
void ExitOnLoadError(const LoadError &err);                       // the error a loop stopped at, as the reference prints it (after the output before it)

// ---- gtx_host_regionops.cpp: what the drivers that print a line per region share (with gtx_host_blocks.cpp) ------------------
void UpdateThick(PairQuery &q);                                   // GenomicRegionBED::UpdateThick (:2326-2333)
// GenomicRegionBED::Print (:2188-2218) of the region as it is now, appended to out; "exons cannot overlap!" ends the run behind the
// half-printed line
void Print(std::string &out, const PairQuery &q, long int n_line);
// what a loop does with one region and its raw line: its output appended to `out`
typedef std::function<void(std::string &out, GenomicRegion *r, const std::string &raw)> Renderer;
// the host loop over what is left of the set, region by region; an input error ends it behind the output in front of the line
void HostLoop(GenomicRegionSet *set, const Renderer &render);
// the same for the lines of one block of text that came back from the device, with their own line numbers
void HostBlock(const char *text, size_t bytes, long int first_line, const Renderer &render, const std::string &format = "BED");
int WriteSink(void *user, const char *text, size_t bytes);       // a gtx_lines_sink that writes to the FILE * in `user`

// ---- gtx_host_device.cpp: the GPU context shared by the classes, the page-locked pool, the hand-over ------------------------
inline void Mark(const char *what) { GtxMark(what); }
void GtxWarmUp();                                                 // HIP start-up on its own thread, from the first region set on
void StdoutIsOurs();                                              // nothing may reach stdout before RCCL's banner is over
gtx_group *Devices();                                             // joins the start-up thread; exits with its error
void CheckGrp(gtx_group *g, int rc);                              // rc != GTX_OK: the group's last error, exit(1)
void DieGtx(gtx_ctx *ctx, int rc);                                // rc != GTX_OK: the context's last error, exit(1)

// Page-locked batch buffers for the bulk packer (gtxhost::BatchArena): two of them, filled in turn by DrainSet -- the packer
// threads write the packed triples where the DMA engine reads them (gtx_host_alloc memory skips the library's staging copy, and
// the call returns with the copy in flight: the contract of include/gtx.h is "untouched until the NEXT call has returned", which
// two alternating buffers satisfy).  Made by the start-up thread behind the loading of the reference set.
struct BatchPool { void *buf[2]; bool used[2]; gtx_ctx *owner; };
extern BatchPool g_pool;
extern std::future<void> g_pool_future;
extern const size_t kPoolBytes;                                   // what BedPacker::NextBatch reserves for a batch

// GTX_TEXT_ON_DEVICE: 0 never; 1 whenever the input qualifies (tests); not set: inputs of 32 MB or more (threshold_bytes: 1 when forced)
struct TextDevicePolicy { bool never, forced; size_t threshold_bytes; };
const TextDevicePolicy &TextPolicy();

// What DrainSet needs to have a streamed BED file tokenised on the device (gtx_count_add_text, include/gtx.h) instead of parsing it
// here: add(text, bytes, lines, rules) -> ticket, and needs_host(ticket).  The device takes the plain case only; a block with
// anything else in it comes back and is packed here, with the reference's reading of it and the reference's errors.
struct TextSink {
  std::function<bool()> usable;                                   // (asked behind prep(): one GPU)
  std::function<int(const char *, size_t, int64_t, const gtx_text_rules &, uint32_t)> add;   // (the last argument: GTX_TEXT_SAM, GTX_TEXT_GFF or 0, to go with the call's flags)
  std::function<bool(int)> needs_host;
};

// Packs the rest of a query/input set batch by batch and hands every batch to `sink`, in order; `prep` (wait for the HIP context
// that the start-up thread is making, gtx_set_refs, *_begin) runs first.  In-memory sets are walked region by region with the same
// rules.  on_error (may be empty): called with the packer's error instead of dying with it, after the batch in hand -- which, under
// PackOptions::keep_prefix_on_error, holds the regions of the lines in front of the offending one -- has gone to `sink`; nothing
// more is packed.  (Plain std::function arguments: the sink runs once per 8 M reads, the indirection costs nothing.)
extern std::atomic<bool> g_drain_stop;                            // set by a sink that has seen enough (an error it will raise after DrainSet): no more batches
void DrainSet(GenomicRegionSet *set, PackOptions opt, const std::function<void()> &prep, const std::function<void(const PackedBatch &)> &sink,
              const TextSink *text_sink = NULL, const std::function<void(const PackError &)> &on_error = std::function<void(const PackError &)>());

// The two-block text pump of the device tokenizer's users (DrainSet, genomic_subset's text path): blocks of complete lines are read
// straight into the two page-locked buffers of the pool, which it holds while it lives, two blocks in flight: block i's verdict is
// collected before block i+2 is read over it.  add(block, rules) hands a block to the device -- rules carry the key of the line
// before it, for the order check at the seam -- and returns its ticket (negative: not handed over); settle(block, ticket) collects
// the verdict and says whether to go on.  Either may set `stop`.  What a refused block means is the caller's business.
struct TextPump {
  typedef BedPacker::TextBlock Block;
  TextPump(BedPacker &packer, const PackOptions &opt);
  ~TextPump();
  std::function<int(const Block &, const gtx_text_rules &)> add;
  std::function<bool(const Block &, int)> settle;
  bool one_at_a_time = false;                                     // every block settled before the next one is read
  bool stop = false;
  Block blk[2];
  void Add(int k);                                                // blk[k] to the device
  void Settle(int k);                                             // the verdict on blk[k], if it is in flight
  void SettleAll() { Settle(0); Settle(1); }
  void Run(int cur);                                              // blocks into slot cur, cur ^ 1, ... until the text ends or `stop`; then the verdicts still out, the older block's first
 private:
  BedPacker &packer_;
  std::vector<const char *> names_;
  gtx_text_rules rules_;
  int ticket_[2] = {-1, -1};
};

// ---- gtx_host_regionops.cpp: the device text loop of the tools that print lines from lines (with gtx_host_blocks.cpp) ----------
// One GPU, and the page-locked pool is there: what every such tool asks before its own conditions.  (The first thing it does is
// Devices(), before anything is printed: without a GPU the run ends there.)
bool OneGpuWithPool();

// a page-locked buffer for a block's printed text: grown on demand, to need + need / 8, and freed with the loop that owns it
struct PinnedOut {
  char *Reserve(gtx_ctx *ctx, size_t need);                       // at least `need` bytes; dies with the library's error
  ~PinnedOut();
 private:
  gtx_ctx *ctx_ = NULL; char *p_ = NULL; size_t cap_ = 0;
};

// what DeviceTextLoop shows of itself to an `add` that renders a block on its own (the rewrite's short stream): such an add
// settles the pump, counts the block as one that came back and returns a negative ticket
struct LineLoopView { TextPump *pump; BedPacker *packer; const std::string *first; long int *came_back; };

// A tool's side of the loop.  trace: the GTX_TEXT_TRACE line up to the colon; sam / gff: the format of the set's text, for the packer
// and for the blocks that come back; chrom_names: the frozen table's names (bounds; else none).  add: one call of the C ABI, returns
// the ticket.  result: fetches the ticket's block and writes what the device printed to stdout; true: the block came back.
struct LineFamily {
  const char *trace;
  bool sam, gff;
  std::vector<const char *> chrom_names;
  std::function<int(gtx_ctx *, const TextPump::Block &)> add;
  std::function<bool(gtx_ctx *, int ticket, const TextPump::Block &)> result;
  LineLoopView *view;                                             // filled before the first add when not NULL
};
// The set's text block by block through f.add, two blocks in flight, the printed text to stdout in block order through f.result; a
// block that comes back is rendered here (HostBlock with `render`), alone, and the next one goes to the device again.  The line the
// set's constructor has read goes first, as a block of one line.
void DeviceTextLoop(GenomicRegionSet *set, const LineFamily &f, const Renderer &render);

// quick order hint for the kernel choice (a wrong hint only costs speed; the device verifies it and falls back by itself): adjacent
// pairs of packed triples sampled at ~4096 places, with so many descents let through (a batch is a few sorted runs at most, e.g.
// the '+' then the '-' reads).  Each caller keeps its own tolerance: the hint picks a kernel route.
template <class Triples>
bool LooksSorted(const Triples &tri, int tolerated_descents)
{
  const size_t n = tri.size() / 3;
  if (n < 2) return true;
  const size_t stride = n > 4096 ? n / 4096 : 1;
  int descents = 0;
  for (size_t i = 0; i + 1 < n; i += stride) {
    const int32_t *a = &tri[3 * i], *b = a + 3;
    if ((b[0] < a[0] || (b[0] == a[0] && b[1] < a[1])) && ++descents > tolerated_descents) return false;
  }
  return true;
}
// the same hint from the text of a block.  format: GTX_TEXT_SAM, GTX_TEXT_GFF or 0 for BED
bool TextLooksSorted(const char *text, size_t bytes, uint32_t format = 0);

}  // namespace gtx_host
