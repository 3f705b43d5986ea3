// gtx_host_device.cpp -- the GPU side every family of the host class layer shares (gtx_host.h): the start-up thread and the group
// of contexts, the page-locked pool, the hand-over of a set to the device (DrainSet, the text pump), the order hints.
#include "gtx_host.h"

#include <unistd.h>
#include <algorithm>
#include <chrono>

using namespace gtx_host;

// End of a tool's main(): everything is written; what is left at a normal return is freeing a million region
// objects and the HIP runtime's own shutdown (~0.3 s of a 0.8 s run).  The process is about to disappear anyway:
// flush and leave.  A normal return is kept when a profiler is attached (it reports from exit handlers) or when
// GTX_FULL_EXIT is set.
void GtxFinish(int code)
{
  if (getenv("GTX_TIMING")) fprintf(stderr, "[gtx leaving at epoch ms %lld]\n", (long long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count());
  fflush(stdout); fflush(stderr);
  const char *pre = getenv("LD_PRELOAD");
  if (getenv("GTX_FULL_EXIT") || getenv("ROCP_TOOL_LIBRARIES") || getenv("ROCPROFILER_REGISTER_FORCE_LOAD") || getenv("HSA_TOOLS_LIB") ||
      (pre && strstr(pre, "rocprof")))
    return;
  _exit(code);
}
// GTX_TIMING=1: wall-clock marks on stderr (where the end-to-end time of a CLI run goes)
void GtxMark(const char *what)
{
  static const bool on = getenv("GTX_TIMING") != NULL;
  static const auto t0 = std::chrono::steady_clock::now();
  static const bool first = on && fprintf(stderr, "[gtx first mark at epoch ms %lld]\n", (long long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count()) > 0;
  (void)first;
  if (on) fprintf(stderr, "[gtx %8.3f s] %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), what);
}

// ---------------------------------------------------------------------------------------------------
// GPU context shared by the classes
// ---------------------------------------------------------------------------------------------------
// HIP start-up takes ~0.2 s: it runs on its own thread from the first region set on, next to the
// parsing of the reference file (GtxWarmUp), and is joined when the context is first needed.
// The classes drive a gtx_group: one context per GPU (--ngpu N / GTX_NGPU, default 1; devices GTX_DEVICE,
// GTX_DEVICE+1, ...), classes dealt to the GPUs, RCCL reduce of the result vector (include/gtx.h).  A group of one is a
// plain context.
static std::future<gtx_group *> g_group_future;
static std::string g_ctx_error;
static int g_ngpu = 0;                                   // 0 = not set: GTX_NGPU or 1

void GtxSetDevices(int n) { g_ngpu = n; }

// one GPU, and the environment variable `off_switch` is not 0 (0: the per-window loop on the host)
static bool OneGpuAndNotOff(const char *off_switch)
{
  const char *e = getenv(off_switch);
  if (e && atoi(e) == 0) return false;
  int n = g_ngpu;
  if (n <= 0) { const char *g = getenv("GTX_NGPU"); n = g ? atoi(g) : 1; }
  return n <= 1;
}
bool GtxScanFilterOnDevice() { return OneGpuAndNotOff("GTX_SCAN_FILTER_ON_DEVICE"); }
bool GtxPeaksOnDevice() { return OneGpuAndNotOff("GTX_PEAKS_ON_DEVICE"); }
bool GtxScanLinesOnDevice() { return OneGpuAndNotOff("GTX_SCAN_LINES_ON_DEVICE"); }
void GtxScanLinesFallback(const char *why)
{
  const char *e = getenv("GTX_SCAN_LINES_ON_DEVICE");
  if (!e || atoi(e) != 2) return;
  fflush(stdout);
  fprintf(stderr, "Error: GTX_SCAN_LINES_ON_DEVICE=2, and the output lines would fall back to the host loop (%s)!\n", why);
  exit(1);
}

// the page-locked batch buffers (gtx_host.h)
static const size_t kBatchReads = getenv("GTX_HOST_BATCH_READS") && atol(getenv("GTX_HOST_BATCH_READS")) > 0 ? (size_t)atol(getenv("GTX_HOST_BATCH_READS")) : (8u << 20);   // reads per batch handed to the device
const size_t gtx_host::kPoolBytes = (kBatchReads * 3 + (24u << 20)) * sizeof(int32_t);   // what BedPacker::NextBatch reserves for it
BatchPool gtx_host::g_pool = {{NULL, NULL}, {false, false}, NULL};
std::future<void> gtx_host::g_pool_future;

static void *PoolTake(size_t bytes)
{
  if (bytes > kPoolBytes || bytes < kPoolBytes / 2) return NULL;               // the triples of a batch, nothing else
  for (int k = 0; k < 2; k++) if (g_pool.buf[k] && !g_pool.used[k]) { g_pool.used[k] = true; return g_pool.buf[k]; }
  return NULL;
}
static bool PoolGive(void *p)
{
  for (int k = 0; k < 2; k++) if (p && g_pool.buf[k] == p) { g_pool.used[k] = false; return true; }
  return false;
}

static gtx_group *CreateGroup()
{
  int n = g_ngpu;
  if (n <= 0) { const char *e = getenv("GTX_NGPU"); n = e ? atoi(e) : 1; }
  if (n < 1) n = 1;
  const char *d = getenv("GTX_DEVICE");
  const int first = d ? atoi(d) : 0;
  std::vector<int> ids(n);
  const char *rh = getenv("GTX_GROUP_REHEARSE");           // test mode of the library: all members on one device
  for (int i = 0; i < n; i++) ids[i] = first + ((rh && atoi(rh)) ? 0 : i);
  gtx_group *g = gtx_group_create(n, ids.data());
  Mark("HIP context(s) created (start-up thread)");
  if (!g) { g_ctx_error = gtx_group_last_error(NULL); return g; }   // thread-local in the library: copy it out on this thread
  if (getenv("GTX_NO_PINNED_BATCHES") == NULL) {
    // page-locking 2 x 190 MB takes ~70 ms: on a thread of its own, behind the packing of the index set and gtx_set_refs; DrainSet waits for it
    g_pool.owner = gtx_group_ctx(g, 0);
    g_pool_future = std::async(std::launch::async, [] {
      for (int k = 0; k < 2; k++) g_pool.buf[k] = gtx_host_alloc(g_pool.owner, kPoolBytes);    // (NULL: the heap serves)
      Mark("page-locked batch buffers ready (start-up thread)");
      gtxhost::BatchArena::take = PoolTake; gtxhost::BatchArena::give = PoolGive;
    });
  }
  return g;
}

// exit() on an input error may come while the start-up threads are still inside the HIP runtime: they are joined before
// the static destructors (the runtime's own among them) run
static void JoinStartUp()
{
  if (g_group_future.valid()) g_group_future.wait();
  if (g_pool_future.valid()) g_pool_future.wait();
}

// Descriptor 1 points at stderr while the library brings RCCL communicators up on the start-up thread (RCCL prints a banner):
// nothing may reach stdout before that is over.  Only groups of more than one GPU (or the single-member RCCL self-test) make
// communicators.
void gtx_host::StdoutIsOurs()
{
  static bool checked = false;
  if (checked) return;
  checked = true;
  int n = g_ngpu;
  if (n <= 0) { const char *e = getenv("GTX_NGPU"); n = e ? atoi(e) : 1; }
  const char *f = getenv("GTX_GROUP_FORCE_RCCL"), *x = getenv("GTX_GROUP_SELF_EXCHANGE");
  if ((n > 1 || (f && atoi(f)) || (x && atoi(x))) && g_group_future.valid()) g_group_future.wait();
}

void gtx_host::GtxWarmUp()
{
  if (!g_group_future.valid()) {
    atexit(JoinStartUp);
    // (GTX_SYNC_STARTUP=1, diagnostic: bring the device up on the calling thread instead of next to the parsing of the index set)
    g_group_future = std::async(getenv("GTX_SYNC_STARTUP") ? std::launch::deferred : std::launch::async, CreateGroup);
  }
}

gtx_group *gtx_host::Devices()
{
  static gtx_group *grp = NULL;
  if (!grp) {
    GtxWarmUp();
    grp = g_group_future.get();
    if (!grp) { fflush(stdout); fprintf(stderr, "\nError: %s\n", g_ctx_error.c_str()); exit(1); }
  }
  return grp;
}

// the one way the drivers die with the library's error: the group's channel, or a member context's own
static void DieWith(int rc, const char *msg) { fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, msg); exit(1); }
void gtx_host::CheckGrp(gtx_group *g, int rc) { if (rc != GTX_OK) DieWith(rc, gtx_group_last_error(g)); }
void gtx_host::DieGtx(gtx_ctx *ctx, int rc) { if (rc != GTX_OK) DieWith(rc, gtx_last_error(ctx)); }

const TextDevicePolicy &gtx_host::TextPolicy()
{
  static const char *e = getenv("GTX_TEXT_ON_DEVICE");
  static const TextDevicePolicy p = {e && atoi(e) == 0, e && atoi(e) == 1, (e && atoi(e) == 1) ? (size_t)1 : ((size_t)32 << 20)};
  return p;
}

// DrainSet (gtx_host.h).  Two batches in turn, in the two page-locked buffers: one is packed while the device still reads the other
// (the hand-over returns with the copy in flight).  Measured and dropped: packing AHEAD of the hand-over on a helper thread, started
// before the HIP runtime is up -- batches outside the page-locked buffers cost first-touch page faults and a staging copy in the
// library, more page-locked memory to release at exit, and 100 M reads from text came out 10 % slower (0.95 -> 1.06 s on one box).
std::atomic<bool> gtx_host::g_drain_stop(false);

static bool TextOnDevice(GenomicRegionSet *set, const PackOptions &opt, const TextSink *ts)
{
  if (!ts || TextPolicy().never) return false;
  if (set->load_in_memory || (set->format != "BED" && set->format != "SAM" && set->format != "GFF")) return false;
  if (opt.guard || opt.collect_zero_length) return false;                 // (explode_blocks: a 12-column line sends its block back to the packer, which does it)
  if (!g_pool.buf[0] || !g_pool.buf[1] || !ts->usable()) return false;
  // a regular uncompressed file: worth it from 32 MB on.  A stream (stdin / a pipe, a .gz file, a FILE* of the caller's: -1) has no
  // size to go by: it takes the device path, and pump_text hands a first block that turns out to be all there is to the host packer
  const long left = set->StreamBytesLeft();
  return left < 0 || left >= (long)TextPolicy().threshold_bytes;
}

TextPump::TextPump(BedPacker &packer, const PackOptions &opt) : packer_(packer), names_((size_t)opt.chroms->size())
{
  for (int i = 0; i < opt.chroms->size(); i++) names_[i] = opt.chroms->name(i).c_str();
  rules_.chrom_names = names_.empty() ? NULL : names_.data(); rules_.n_chrom = opt.chroms->size();
  rules_.strand_aware = opt.strand_aware; rules_.sorted_rules = opt.mode == gtxhost::PACK_OVERLAPS_SORTED || opt.mode == gtxhost::PACK_SCAN_SORTED; rules_.sorted_by_strand = opt.sorted_by_strand;
  rules_.max_label_value = opt.max_label_value;
  g_pool.used[0] = g_pool.used[1] = true;                        // (the buffers hold text now: a batch packed here takes heap memory)
  packer_.UseTextBuffers((char *)g_pool.buf[0], (char *)g_pool.buf[1], kPoolBytes);
}
TextPump::~TextPump() { g_pool.used[0] = g_pool.used[1] = false; }

void TextPump::Add(int k)
{
  const Block &b = blk[k];
  rules_.have_prev = b.have_prev; rules_.prev_chrom = b.prev_chrom.c_str(); rules_.prev_strand = b.prev_strand; rules_.prev_start = b.prev_start;
  ticket_[k] = add(b, rules_);
}

void TextPump::Settle(int k)
{
  if (ticket_[k] < 0) return;
  const int ticket = ticket_[k];
  ticket_[k] = -1;
  if (!settle(blk[k], ticket)) stop = true;
}

void TextPump::Run(int cur)
{
  for (;; cur ^= 1) {
    Settle(cur);                                                 // (its buffer is about to be read over)
    if (stop || !packer_.NextTextBlock(&blk[cur])) break;
    Add(cur);
    if (stop) break;
    if (one_at_a_time) Settle(cur);
  }
  Settle(cur ^ 1); Settle(cur);
}

void gtx_host::DrainSet(GenomicRegionSet *set, PackOptions opt, const std::function<void()> &prep, const std::function<void(const PackedBatch &)> &sink,
                        const TextSink *text_sink, const std::function<void(const PackError &)> &on_error)
{
  g_drain_stop = false;
  opt.sam = set->format == "SAM";
  opt.gff = set->format == "GFF" && !set->load_in_memory;        // (an in-memory set goes out again as BED lines, below)
  const size_t batch_reads = kBatchReads;
  PackedBatch two[2]; PackError err;
  // (a scanner's batch without a single region for the windows still carries the label values of its lines)
  const bool scan_mode = opt.mode == gtxhost::PACK_SCAN_SORTED || opt.mode == gtxhost::PACK_SCAN_UNSORTED;
  auto worth = [&](const PackedBatch &b) { return !b.empty() || (scan_mode && b.label_sum != 0); };
  auto pump_text = [&](BedPacker &packer) {
    // tokenised and counted on the device; what is not plain is packed here
    TextPump pump(packer, opt);
    PackedBatch batch;
    if (!packer.PackPrimedText(&batch, &err) && !on_error) DiePack(err);
    if (worth(batch)) sink(batch);
    if (err.set) { on_error(err); g_drain_stop = true; return; }
    bool host_only = false, first_block = true;
    long on_device = 0, redone = 0, host_blocks = 0;
    auto pack_here = [&](const TextPump::Block &b, bool older_first) {
      batch.clear();
      packer.PackTextBlock(b, &batch, &err);
      if (err.set && !on_error) { if (older_first) pump.SettleAll(); DiePack(err); }
      if (worth(batch)) sink(batch);
      if (err.set) { on_error(err); g_drain_stop = true; }
    };
    pump.settle = [&](const TextPump::Block &b, int ticket) {
      if (!text_sink->needs_host(ticket)) on_device++;
      else { redone++; pack_here(b, false); }
      return !g_drain_stop;
    };
    pump.add = [&](const TextPump::Block &b, const gtx_text_rules &rules) {
      if (!b.seam_ok) host_only = true;                          // a last line that could not be read: no seam key for the device
      if (first_block && b.bytes < TextPolicy().threshold_bytes && packer.SourceAtEnd()) host_only = true;   // a short stream: the host packer is done before the device has the text
      first_block = false;
      int ticket = -1;
      if (host_only) { host_blocks++; pack_here(b, true); }
      else ticket = text_sink->add(b.text, b.bytes, b.n_lines, rules, opt.sam ? GTX_TEXT_SAM : opt.gff ? GTX_TEXT_GFF : 0u);
      pump.stop = g_drain_stop;
      return ticket;
    };
    pump.one_at_a_time = (bool)on_error;                         // (a caller that goes on after an error wants nothing behind the offending line counted)
    pump.stop = g_drain_stop;
    pump.Run(0);
    if (getenv("GTX_TEXT_TRACE")) fprintf(stderr, "[gtx text] blocks tokenised on the device: %ld, sent back to the host packer: %ld, packed on the host from the start: %ld\n", on_device, redone, host_blocks);
  };
  auto pump = [&](BedPacker &packer, bool prepared = false) {
    if (!prepared) prep();
    if (g_pool_future.valid()) g_pool_future.get();             // the page-locked batch buffers are there
    for (int cur = 0;;) {
      PackedBatch &batch = two[cur];
      bool more = packer.NextBatch(&batch, batch_reads, &err);
      if (g_drain_stop) break;
      if (err.set && !on_error) DiePack(err);
      if (worth(batch)) {
        const auto t0 = std::chrono::steady_clock::now();
        sink(batch); cur ^= 1;
        if (getenv("GTX_PACK_TRACE")) fprintf(stderr, "[sink] %zu reads handed over in %.1f ms\n", batch.tri.size() / 3, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      }
      if (err.set) { on_error(err); break; }
      if (!more) break;
    }
  };
  if (!set->load_in_memory && set->format == "GTX") {
    long int at = 0;
    const gtxhost::GtxView *view = set->DetachPacked(&at);
    BedPacker packer(view, opt);
    packer.SkipRecords((uint64_t)at);
    pump(packer);
    return;
  }
  if (!set->load_in_memory) {
    std::string first; long int first_no = 0;
    LineSource *src = NULL;
    bool on_device = false;
    if (text_sink) {                                             // the decision needs the page-locked buffers and the device: made behind prep()
      prep();
      if (g_pool_future.valid()) g_pool_future.get();
      on_device = TextOnDevice(set, opt, text_sink);
    }
    src = set->DetachStream(&first, &first_no);
    BedPacker packer(src, opt);
    if (first_no > 0) packer.Prime(first, first_no);
    if (on_device) pump_text(packer); else pump(packer, text_sink != NULL);
    return;
  }
  // in-memory set: re-emit its regions as lines through the same packer rules
  if (opt.strand_aware) CheckGffStrands(set);
  std::string text;
  for (GenomicRegion *r = set->Get(); r != NULL; r = set->Next()) {
    GenomicInterval *i = r->I.front();
    if (r->I.size() > 1) {                                  // a multi-interval region: its envelope under -gaps, its intervals one by one for coverage
      if (!opt.match_gaps && !opt.explode_blocks && !opt.collect_blocks) r->PrintError("multi-interval (BED12) regions are outside the MI355X counting path (except genomic_overlaps count, coverage and density)!");
      if (!r->IsCompatibleSortedAndNonoverlapping()) r->PrintError("query regions should be compatible, sorted and non-overlapping!");
    }
    char buf[64];
    if (opt.collect_blocks && r->I.size() > 1) {               // as a 12-column line: the packer lists its intervals
      text += i->CHROMOSOME; text += '\t';
      snprintf(buf, sizeof buf, "%ld\t%ld\t", i->START - 1, r->I.back()->STOP); text += buf;
      text += r->LABEL; text += "\t0\t"; text += i->STRAND; text += "\t0\t0\t0\t";
      snprintf(buf, sizeof buf, "%zu\t", r->I.size()); text += buf;
      for (GenomicIntervalSet::iterator b = r->I.begin(); b != r->I.end(); b++) { snprintf(buf, sizeof buf, "%ld,", (*b)->STOP - (*b)->START + 1); text += buf; }
      text += '\t';
      for (GenomicIntervalSet::iterator b = r->I.begin(); b != r->I.end(); b++) { snprintf(buf, sizeof buf, "%ld,", (*b)->START - i->START); text += buf; }
      text += '\n';
      continue;
    }
    if (opt.explode_blocks && r->I.size() > 1) {
      for (GenomicIntervalSet::iterator b = r->I.begin(); b != r->I.end(); b++) {
        text += i->CHROMOSOME; text += '\t';
        snprintf(buf, sizeof buf, "%ld\t%ld\t", (*b)->START - 1, (*b)->STOP); text += buf;
        text += r->LABEL; text += "\t0\t"; text += i->STRAND; text += '\n';
      }
      continue;
    }
    text += i->CHROMOSOME; text += '\t';
    snprintf(buf, sizeof buf, "%ld\t%ld\t", i->START - 1, r->I.back()->STOP); text += buf;
    // (a GFF feature of another strand byte than '+' or '-' gets this far only when the strand is ignored: any legal BED strand will do)
    text += r->LABEL; text += "\t0\t"; text += (set->format == "GFF" && i->STRAND != '-') ? '+' : i->STRAND; text += '\n';
  }
  BedPacker packer((LineSource *)NULL, opt);
  packer.PrimeBlock(text, 1);
  pump(packer);
}

// the same hint from the text of a block: pairs of adjacent lines at ~4096 places, (chromosome token, start column) compared.
// format: GTX_TEXT_SAM, GTX_TEXT_GFF or 0 for BED
bool gtx_host::TextLooksSorted(const char *text, size_t bytes, uint32_t format)
{
  const bool sam = format == GTX_TEXT_SAM, gff = format == GTX_TEXT_GFF;
  if (bytes < 64) return true;
  const size_t stride = bytes > (4096u * 64u) ? bytes / 4096 : 64;
  int descents = 0;
  auto key = [&](const char *l, const char *e, const char **tok, size_t *len, long *start) {
    if (sam) {                                                     // SAM: (RNAME, POS), columns 3 and 4
      for (int k = 0; k < 2 && l; k++) { l = (const char *)memchr(l, '\t', (size_t)(e - l)); if (l) l++; }
      if (!l) return false;
    }
    const char *t = (const char *)memchr(l, '\t', (size_t)(e - l));
    if (!t) return false;
    *tok = l; *len = (size_t)(t - l);
    if (gff) {                                                     // GFF: (seqname, START), columns 1 and 4
      for (int k = 0; k < 2 && t; k++) t = (const char *)memchr(t + 1, '\t', (size_t)(e - t - 1));
      if (!t) return false;
    }
    *start = atol(t + 1);
    return true;
  };
  for (size_t at = 0; at + 2 < bytes; at += stride) {
    const char *a = (const char *)memchr(text + at, '\n', bytes - at);
    if (!a || a + 1 >= text + bytes) break;
    a++;
    const char *ae = (const char *)memchr(a, '\n', (size_t)(text + bytes - a));
    if (!ae || ae + 1 >= text + bytes) break;
    const char *b = ae + 1, *be = (const char *)memchr(b, '\n', (size_t)(text + bytes - b));
    if (!be) break;
    const char *ta, *tb; size_t la, lb; long sa, sb;
    if (!key(a, ae, &ta, &la, &sa) || !key(b, be, &tb, &lb, &sb)) continue;
    const int d = memcmp(ta, tb, std::min(la, lb));
    const bool before = d ? d > 0 : (la != lb ? la > lb : sb < sa);
    if (before && ++descents > 2) return false;
  }
  return true;
}
