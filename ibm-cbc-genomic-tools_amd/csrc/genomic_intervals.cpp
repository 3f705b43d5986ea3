// genomic_intervals.cpp -- see genomic_intervals.h.  Host side only: ingest, option semantics,
// error messages; every reduction is a call into libgtx.so (include/gtx.h).
#include "genomic_intervals.h"

#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <functional>
#include <map>
#include <set>
#include <shared_mutex>
#include <sys/mman.h>
#include <stdint.h>
#include <condition_variable>
#include <mutex>
#include <atomic>
#include <future>
#include <thread>
#include <iostream>

#include "gtx.h"
#include "gtx_bed.h"

using gtxhost::BedPacker;
using gtxhost::ChromTable;
using gtxhost::LineSource;
using gtxhost::PackedBatch;
using gtxhost::PackError;
using gtxhost::PackOptions;

bool _MESSAGES_ = false;

// GTX_TIMING=1: wall-clock marks on stderr (where the end-to-end time of a CLI run goes)
#include <chrono>
void GtxMark(const char *what);
static void Mark(const char *what) { GtxMark(what); }

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
void GtxMark(const char *what)
{
  static const bool on = getenv("GTX_TIMING") != NULL;
  static const auto t0 = std::chrono::steady_clock::now();
  static const bool first = on && fprintf(stderr, "[gtx first mark at epoch ms %lld]\n", (long long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count()) > 0;
  (void)first;
  if (on) fprintf(stderr, "[gtx %8.3f s] %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), what);
}

// ---- memory of region objects built in parallel (see genomic_intervals.h) ----
namespace {
struct Block { char *cur = NULL, *end = NULL; std::vector<std::pair<void *, size_t> > owned; };
thread_local Block *tls_block = NULL;
std::shared_timed_mutex g_blocks_mu;
std::vector<std::pair<uintptr_t, uintptr_t> > g_blocks;            // [first, last) of every live block, sorted

void BlockGrow(Block *b, size_t at_least)
{
  const size_t want = std::max(at_least, (size_t)4 << 20), bytes = (want + 4095) & ~(size_t)4095;
  void *p = mmap(NULL, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_POPULATE, -1, 0);   // (pre-faulted: one call instead of a fault per page)
  if (p == MAP_FAILED) { fprintf(stderr, "Error: out of memory!\n"); exit(1); }
  b->cur = (char *)p; b->end = b->cur + bytes; b->owned.push_back(std::make_pair(p, bytes));
  std::unique_lock<std::shared_timed_mutex> lk(g_blocks_mu);
  g_blocks.insert(std::upper_bound(g_blocks.begin(), g_blocks.end(), std::make_pair((uintptr_t)p, (uintptr_t)0)), std::make_pair((uintptr_t)p, (uintptr_t)p + bytes));
}

bool InBlocks(const void *p)
{
  std::shared_lock<std::shared_timed_mutex> lk(g_blocks_mu);
  if (g_blocks.empty()) return false;
  auto it = std::upper_bound(g_blocks.begin(), g_blocks.end(), std::make_pair((uintptr_t)p, ~(uintptr_t)0));
  if (it == g_blocks.begin()) return false;
  --it;
  return (uintptr_t)p >= it->first && (uintptr_t)p < it->second;
}

void BlocksRelease(std::vector<std::pair<void *, size_t> > &owned)
{
  if (owned.empty()) return;
  std::unique_lock<std::shared_timed_mutex> lk(g_blocks_mu);
  for (auto &o : owned) {
    auto it = std::lower_bound(g_blocks.begin(), g_blocks.end(), std::make_pair((uintptr_t)o.first, (uintptr_t)0));
    if (it != g_blocks.end() && it->first == (uintptr_t)o.first) g_blocks.erase(it);
    munmap(o.first, o.second);
  }
  owned.clear();
}
}  // namespace

void *GtxRegionAlloc(size_t bytes)
{
  Block *b = tls_block;
  if (!b) return ::operator new(bytes);
  bytes = (bytes + 15) & ~(size_t)15;
  if ((size_t)(b->end - b->cur) < bytes) BlockGrow(b, bytes);
  void *p = b->cur; b->cur += bytes;
  return p;
}

void GtxRegionFree(void *p) { if (p && !InBlocks(p)) ::operator delete(p); }

static char *CopyString(const char *s) { size_t n = strlen(s) + 1; char *p = (char *)GtxRegionAlloc(n); memcpy(p, s, n); return p; }

// The threads that build an in-memory set (GenomicRegionSet::Init) must not exit() on a malformed line -- another thread may hold
// an earlier one: they note the error here and unwind; Init raises the one with the smallest line number, as the reference's
// line-by-line reader would have.
struct LoadError { bool set = false; long int line = 0; std::string msg; bool with_prefix = true; };
struct LoadAbort {};
static thread_local LoadError *tls_load_error = NULL;

static void DieLine(long int n_line, const std::string &msg)
{
  if (tls_load_error) { tls_load_error->set = true; tls_load_error->line = n_line; tls_load_error->msg = msg; tls_load_error->with_prefix = true; throw LoadAbort(); }
  fflush(stdout);
  fprintf(stderr, "\n");
  fprintf(stderr, "Error: Line %ld: %s\n", n_line, msg.c_str());
  exit(1);
}

static void DiePack(const PackError &e)
{
  if (e.no_prefix) { fflush(stdout); fprintf(stderr, "%s\n", e.msg.c_str()); exit(1); }
  DieLine(e.line, e.msg);
}

// ---------------------------------------------------------------------------------------------------
// GenomicInterval / GenomicRegion
// ---------------------------------------------------------------------------------------------------
GenomicInterval::GenomicInterval(const char *chromosome, char strand, long int start, long int stop, long int n_line)
{
  CHROMOSOME = CopyString(chromosome); STRAND = strand; START = start; STOP = stop; this->n_line = n_line;
}

GenomicInterval::~GenomicInterval() { GtxRegionFree(CHROMOSOME); }

void GenomicInterval::PrintInterval() { printf("%s %c %ld %ld", CHROMOSOME, STRAND, START, STOP); }

int GenomicInterval::CalcDirection(GenomicInterval *i, bool sorted_by_strand)
{
  const int by_chrom = strcmp(CHROMOSOME, i->CHROMOSOME);
  if (by_chrom != 0) return by_chrom;
  if (sorted_by_strand && STRAND != i->STRAND) return STRAND - i->STRAND;
  if (i->STOP < START) return 1;
  if (STOP < i->START) return -1;
  return 0;
}
void GenomicInterval::PrintInterval(FILE *f) { fprintf(f, "%s %c %ld %ld", CHROMOSOME, STRAND, START, STOP); }

bool GenomicInterval::OverlapsWith(GenomicInterval *i, bool ignore_strand)
{
  if (strcmp(CHROMOSOME, i->CHROMOSOME) != 0) return false;
  if (!ignore_strand && STRAND != i->STRAND) return false;
  return !(START > i->STOP || STOP < i->START);
}

long int GenomicInterval::CalcOverlap(GenomicInterval *i, bool ignore_strand)
{
  if (strcmp(CHROMOSOME, i->CHROMOSOME) != 0) return 0;
  if (!ignore_strand && STRAND != i->STRAND) return 0;
  const long int y = std::min(STOP, i->STOP) - std::max(START, i->START) + 1;
  return y > 0 ? y : 0;
}

GenomicRegion::GenomicRegion() : n_line(0), LABEL(NULL) {}

GenomicRegion::~GenomicRegion()
{
  GtxRegionFree(LABEL);
  for (size_t k = 0; k < I.size(); k++) delete I[k];
}

void GenomicRegion::PrintError(std::string error_msg) { DieLine(n_line, error_msg); }

size_t GenomicRegion::GetSize(bool skip_gaps)
{
  if (!skip_gaps) return (size_t)(I.back()->STOP - I.front()->START + 1);
  size_t size = 0;
  for (size_t k = 0; k < I.size(); k++) size += I[k]->GetSize();
  return size;
}

long int GenomicRegion::GetLabelValue(long int max_label_value)
{
  if (max_label_value <= 1) return 1;
  return std::min(max_label_value, atol(LABEL));
}

bool GenomicRegion::IsBefore(GenomicRegion *r, bool sorted_by_strand)
{
  GenomicInterval *a = I.front(), *b = r->I.front();
  int d = strcmp(a->CHROMOSOME, b->CHROMOSOME);
  if (d != 0) return d < 0;
  if (sorted_by_strand && a->STRAND != b->STRAND) return a->STRAND < b->STRAND;
  return a->START < b->START;
}

bool GenomicRegion::IsCompatibleSortedAndNonoverlapping()
{
  for (size_t k = 1; k < I.size(); k++) {
    if (strcmp(I[0]->CHROMOSOME, I[k]->CHROMOSOME) != 0 || I[0]->STRAND != I[k]->STRAND) return false;
    if (I[k]->START < I[k - 1]->START) return false;
  }
  for (size_t k = 1; k < I.size(); k++) if (I[k]->START <= I[k - 1]->STOP) return false;
  return true;
}

bool GenomicRegion::OverlapsWith(GenomicRegion *r, bool ignore_strand)
{
  for (size_t a = 0; a < I.size(); a++)
    for (size_t b = 0; b < r->I.size(); b++) if (I[a]->OverlapsWith(r->I[b], ignore_strand)) return true;
  return false;
}

long int GenomicRegion::CalcOverlap(GenomicRegion *r, bool ignore_strand)
{
  long int y = 0;
  for (size_t a = 0; a < I.size(); a++)
    for (size_t b = 0; b < r->I.size(); b++) y += I[a]->CalcOverlap(r->I[b], ignore_strand);
  return y;
}

int GenomicRegion::CalcDirection(GenomicRegion *r, bool sorted_by_strand)
{
  const int by_chrom = strcmp(I.front()->CHROMOSOME, r->I.front()->CHROMOSOME);
  if (by_chrom != 0) return by_chrom;
  if (sorted_by_strand && I.front()->STRAND != r->I.front()->STRAND) return I.front()->STRAND - r->I.front()->STRAND;
  if (r->I.back()->STOP < I.front()->START) return 1;
  if (I.back()->STOP < r->I.front()->START) return -1;
  return 0;
}

GenomicRegionBED::GenomicRegionBED(char *inp, long int n_line)
{
  this->n_line = n_line;
  gtxhost::BedFields f; char *bad = NULL;
  gtxhost::BedStatus st = gtxhost::ParseBedLine(inp, &f, &bad);
  if (st == gtxhost::BED_TOO_FEW_TOKENS) PrintError("number of tokens should be at least 3 for BED format!");
  if (st == gtxhost::BED_BAD_STRAND) {
    if (tls_load_error) { tls_load_error->set = true; tls_load_error->line = n_line; tls_load_error->msg = std::string("Error: invalid strand '") + bad + "'!"; tls_load_error->with_prefix = false; throw LoadAbort(); }
    fflush(stdout); std::cerr << "Error: invalid strand '" << bad << "'!\n"; exit(1);
  }
  n_tokens = f.n_tokens;
  LABEL = CopyString(f.label ? f.label : "_");
  if (n_tokens != 12) { I.push_back(new GenomicInterval(f.chrom, f.strand, f.start, f.stop, n_line)); return; }
  std::vector<long> iv; gtxhost::BedBlocks(f, &iv);                                     // :2174-2181
  for (size_t k = 0; k + 1 < iv.size(); k += 2) I.push_back(new GenomicInterval(f.chrom, f.strand, iv[k], iv[k + 1], n_line));
  if (I.empty()) PrintError("BED12 line without blocks!");
}

GenomicRegionSAM::GenomicRegionSAM(char *inp, long int n_line)
{
  this->n_line = n_line;
  CIGAR = RNEXT = SEQ = QUAL = OPTIONAL = NULL;
  gtxhost::SamFields f; std::vector<long> iv; std::string msg;
  if (gtxhost::ParseSamLine(inp, &f, &iv, &msg) != gtxhost::SAM_OK) PrintError(msg);
  n_tokens = f.n_tokens;
  LABEL = CopyString(f.qname);
  FLAG = f.flag; MAPQ = f.mapq; PNEXT = f.pnext; TLEN = f.tlen;
  CIGAR = CopyString(f.cigar_text.c_str()); RNEXT = CopyString(f.rnext); SEQ = CopyString(f.seq); QUAL = CopyString(f.qual);
  OPTIONAL = f.optional ? CopyString(f.optional) : NULL;
  for (size_t k = 0; k + 1 < iv.size(); k += 2) I.push_back(new GenomicInterval(f.rname, f.strand, iv[k], iv[k + 1], n_line));
}

GenomicRegionSAM::~GenomicRegionSAM()
{
  GtxRegionFree(CIGAR); GtxRegionFree(RNEXT); GtxRegionFree(SEQ); GtxRegionFree(QUAL); GtxRegionFree(OPTIONAL);
}

GenomicRegionGFF::GenomicRegionGFF(char *inp, long int n_line)
{
  this->n_line = n_line;
  SOURCE = FEATURE = SCORE = COMMENT = NULL; FRAME = 0;
  gtxhost::GffFields f; std::string msg;
  if (gtxhost::ParseGffLine(inp, &f, &msg) != gtxhost::GFF_OK) PrintError(msg);
  n_tokens = f.n_tokens;
  LABEL = CopyString(f.label ? f.label : "_");
  SOURCE = CopyString(f.source); FEATURE = CopyString(f.feature); SCORE = CopyString(f.score); FRAME = f.frame;
  COMMENT = f.comment ? CopyString(f.comment) : NULL;
  I.push_back(new GenomicInterval(f.seqname, f.strand, f.start, f.stop, n_line));
}

GenomicRegionGFF::~GenomicRegionGFF()
{
  GtxRegionFree(SOURCE); GtxRegionFree(FEATURE); GtxRegionFree(SCORE); GtxRegionFree(COMMENT);
}

// a strand-aware run over the regions of an in-memory GFF set: a strand byte other than '+' or '-' is an input error at its line
// (the engine has two strand classes per chromosome; see gtxhost::GffStrandMessage).  Call before anything renumbers n_line.
static void CheckGffStrands(GenomicRegionSet *set)
{
  if (set->format != "GFF" || !set->load_in_memory) return;
  for (long int k = 0; k < set->n_regions; k++) {
    const char s = set->R[k]->I.front()->STRAND;
    if (s != '+' && s != '-') set->R[k]->PrintError(gtxhost::GffStrandMessage(s));
  }
}

// ---------------------------------------------------------------------------------------------------
// GenomicRegionSet
// ---------------------------------------------------------------------------------------------------
void StdoutIsOurs();   // (below, with the GPU start-up)
static bool g_accept_sam = true, g_accept_gff = true;            // (the two formats only the reductions read)
void GtxAcceptSAM(bool on) { g_accept_sam = on; g_accept_gff = on; }   // (the drivers that print lines refuse both)
bool GtxAcceptGFF(bool on) { const bool was = g_accept_gff; g_accept_gff = on; return was; }

GenomicRegionSet::GenomicRegionSet(char *file, unsigned long int buffer_size, bool verbose, bool load_in_memory, bool hide_header)
{
  this->file = file == NULL ? NULL : CopyString(file); this->file_ptr = NULL;
  this->buffer_size = buffer_size;
  this->verbose = verbose;
  this->from_stdin = file == NULL;
  this->load_in_memory = from_stdin ? false : load_in_memory;
  this->hide_header = hide_header;
  this->src = NULL; this->packed = NULL; this->R = NULL; this->n_regions = 0; this->r_index = 0;
  Init();
}

GenomicRegionSet::GenomicRegionSet(FILE *file_ptr, unsigned long int buffer_size, bool verbose, bool load_in_memory, bool hide_header)
{
  this->file = NULL; this->file_ptr = file_ptr;
  this->buffer_size = buffer_size;
  this->verbose = verbose;
  this->from_stdin = file_ptr == stdin;
  this->load_in_memory = from_stdin ? false : load_in_memory;
  this->hide_header = hide_header;
  this->src = NULL; this->packed = NULL; this->R = NULL; this->n_regions = 0; this->r_index = 0;
  Init();
}

GenomicRegionSet::GenomicRegionSet(const std::vector<GenomicRegion *> &regions)
{
  file = NULL; file_ptr = NULL; buffer_size = 0; verbose = false; from_stdin = false; load_in_memory = true; hide_header = true;
  src = NULL; packed = NULL; r_index = 0;
  n_regions = (long int)regions.size();
  R = n_regions > 0 ? new GenomicRegion *[n_regions] : NULL;
  for (long int k = 0; k < n_regions; k++) R[k] = regions[k];
  format = n_regions > 0 ? "REG" : "EMPTY";
}

GenomicRegionSet::~GenomicRegionSet()
{
  GtxRegionFree(file);
  delete src;
  delete packed;
  if (R) {
    long int n = load_in_memory ? n_regions : 1;
    for (long int k = 0; k < n; k++) delete R[k];
    delete[] R;
  }
  BlocksRelease(blocks_);
  if (load_in_memory) Mark("GenomicRegionSet (in memory): released");
}

void GenomicRegionSet::PrintError(std::string error_msg)
{
  fflush(stdout);
  fprintf(stderr, "\n");
  fprintf(stderr, "Error: %s\n", error_msg.c_str());
  exit(1);
}

// genomic_intervals.cpp:3736-3759: by the number of TAB-separated tokens of the first data line (SAM: 11 or more, GFF: 8 to 10, a 6th
// token without '+' or '-')
void GenomicRegionSet::DetectFormat(const char *line)
{
  if (line[0] == '>' || line[0] == '@' || (line[0] == '#' && line[1] == '#')) PrintError("unsupported input format!\n");
  int nt = gtxhost::CountTokensLike(line, '\t');
  bool bed = nt == 1 || (nt >= 3 && nt <= 6);
  if (!bed && nt >= 6) {
    std::string copy(line);
    const char *p = copy.c_str(); int tabs = 0;
    while (*p && tabs < 5) { if (*p == '\t') tabs++; p++; }
    std::string tok(p, strcspn(p, "\t"));
    bed = tok.find('+') != std::string::npos || tok.find('-') != std::string::npos;
  }
  if (!bed && g_accept_sam && gtxhost::LooksLikeSam(line)) { format = "SAM"; return; }
  if (!bed && g_accept_gff && gtxhost::LooksLikeGff(line)) { format = "GFF"; return; }
  if (!bed) PrintError("unsupported input format!\n");     // REG is outside the path
  format = "BED";
}

GenomicRegion *GenomicRegionSet::CreateRegion(char *line, long int n_line)
{
  if (format == "SAM") return new GenomicRegionSAM(line, n_line);
  if (format == "GFF") return new GenomicRegionGFF(line, n_line);
  return new GenomicRegionBED(line, n_line);
}

void GtxWarmUp();

void GenomicRegionSet::Init()
{
  if (getenv("GTX_NO_WARMUP") == NULL) GtxWarmUp();
  Mark(load_in_memory ? "GenomicRegionSet (in memory): open" : "GenomicRegionSet (stream): open");
  std::string err;
  if (file_ptr == NULL && gtxhost::GtxView::IsGtx(file)) {
    // a packed region file: no text to tokenise; regions are made from its records on demand
    packed = gtxhost::GtxView::Open(file, &err);
    if (!packed) { fprintf(stderr, "%s\n", err.c_str()); exit(1); }
    format = packed->n ? "GTX" : "EMPTY";
    r_index = 0;
    if (load_in_memory) {
      n_regions = (long int)packed->n;
      R = n_regions > 0 ? new GenomicRegion *[n_regions] : NULL;
      for (long int k = 0; k < n_regions; k++) R[k] = PackedRegion(k);
    } else if (packed->n) {
      n_regions = 1;
      R = new GenomicRegion *[1];
      R[0] = PackedRegion(0);
    }
    return;
  }
  src = file_ptr ? LineSource::FromFile(file_ptr) : LineSource::Open(file, &err);
  if (!src) { fprintf(stderr, "%s\n", err.c_str()); exit(1); }
  char *line = src->Next();
  bool sam_header = false;
  if (line && line[0] == '@' && g_accept_sam) {                 // a SAM header (ProcessFileHeader :3721-3724): echoed unless hidden
    sam_header = true;
    while (line && line[0] == '@') {
      if (!hide_header) { StdoutIsOurs(); printf("%s\n", line); }
      line = src->Next();
    }
  }
  bool gff_header = false;
  if (line && line[0] == '#' && line[1] == '#' && g_accept_gff) {   // a GFF header (ProcessFileHeader :3725-3728): the file is GFF whatever follows;
    gff_header = true;                                          // the leading run of '##' lines is echoed unless hidden (a later one is a data line)
    while (line && line[0] == '#' && line[1] == '#') {
      if (!hide_header) { StdoutIsOurs(); printf("%s\n", line); }
      line = src->Next();
    }
  }
  while (!sam_header && !gff_header && line && (strncmp(line, "browser ", 8) == 0 || strncmp(line, "track ", 6) == 0)) {
    if (!hide_header) { StdoutIsOurs(); printf("%s\n", line); }
    line = src->Next();
  }
  if (!line) { format = "EMPTY"; n_regions = 0; }
  else if (sam_header) format = "SAM";
  else if (gff_header) format = "GFF";
  else DetectFormat(line);

  if (load_in_memory) {
    // The first line here, the rest in blocks of complete lines, each block cut at line ends into one piece per thread: the
    // region objects (five small allocations each) are what the load costs, and the allocator scales with the threads
    // (1 M regions: 0.23 s on one thread).  The set is the same objects in the same order; a malformed line is reported as the
    // line-by-line reader would have met it -- the first one in the file.
    std::vector<GenomicRegion *> regs;
    if (line) regs.push_back(CreateRegion(line, src->line_no()));
    // Four threads, not all of them: this runs while the start-up thread brings up the HIP runtime, and a process that had many
    // threads running then takes 0.15-0.2 s longer to go away at exit (measured on the MI355X boxes, 16 threads against 4: every
    // run against none; where the time goes inside the driver's teardown was not found).  Four are enough: the runtime is what the
    // set's caller waits for anyway.
    const int T = getenv("GTX_LOAD_THREADS") && atoi(getenv("GTX_LOAD_THREADS")) > 0 ? atoi(getenv("GTX_LOAD_THREADS")) : std::min(gtxhost::WorkerThreads(), 4);
    std::vector<char> block; char *view = NULL; long first_line = 0;
    size_t got;
    while (line && (got = src->NextBlockView(block, &view, (size_t)64 << 20, &first_line)) > 0) {
      struct Piece { char *b, *e; long lines = 0, first = 0; std::vector<GenomicRegion *> out; LoadError err; Block mem; };
      std::vector<Piece> pc((size_t)std::max(1, std::min<int>(T, (int)(got / (256u << 10)) + 1)));
      char *end = view + got;
      for (size_t t = 0; t < pc.size(); t++) {
        char *b = t == 0 ? view : pc[t - 1].e, *e = t + 1 == pc.size() ? end : view + got * (t + 1) / pc.size();
        if (e < b) e = b;
        while (e < end && e > view && e[-1] != '\n') e++;                   // up to the end of the line it falls into
        pc[t].b = b; pc[t].e = e;
      }
      auto count = [&](size_t t) { pc[t].lines = gtxhost::CountNewlines(pc[t].b, pc[t].e); };
      auto build = [&](size_t t) {
        Piece &p = pc[t];
        p.out.reserve((size_t)p.lines);
        const auto t0 = std::chrono::steady_clock::now();
        BlockGrow(&p.mem, (size_t)p.lines * 176 + (size_t)(p.e - p.b) / 8 + 4096);   // a region (64 B), an interval (48), the vector's slot (16), two strings (more: another block)
        const auto t1 = std::chrono::steady_clock::now();
        tls_block = &p.mem;
        tls_load_error = &p.err;
        long no = p.first;
        try {
          for (char *q = p.b; q < p.e; no++) {
            char *nl = (char *)memchr(q, '\n', (size_t)(p.e - q));
            if (!nl) break;                                                // (cannot happen: pieces end at line ends)
            *nl = 0;
            p.out.push_back(CreateRegion(q, no));
            q = nl + 1;
          }
        } catch (const LoadAbort &) {}
        tls_load_error = NULL; tls_block = NULL;
        if (getenv("GTX_PACK_TRACE")) fprintf(stderr, "[load] piece %zu: %ld lines, block %.1f ms, objects %.1f ms\n", t, p.lines, std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
      };
      auto run = [&](const std::function<void(size_t)> &f) { gtxhost::ParallelFor((int)pc.size(), [&](int t) { f((size_t)t); }); };
      const auto tA = std::chrono::steady_clock::now();
      run(count);
      long total = 0;
      for (auto &p : pc) { p.first = first_line + total; total += p.lines; }
      src->AdvanceLines(total);
      const auto tB = std::chrono::steady_clock::now();
      run(build);
      const auto tC = std::chrono::steady_clock::now();
      if (getenv("GTX_PACK_TRACE")) fprintf(stderr, "[load] %zu pieces: count %.1f ms, build %.1f ms\n", pc.size(), std::chrono::duration<double, std::milli>(tB - tA).count(), std::chrono::duration<double, std::milli>(tC - tB).count());
      for (auto &p : pc) {
        blocks_.insert(blocks_.end(), p.mem.owned.begin(), p.mem.owned.end());
        regs.insert(regs.end(), p.out.begin(), p.out.end());
        if (p.err.set) {                                                    // the pieces are in file order: this is the first bad line
          if (p.err.with_prefix) DieLine(p.err.line, p.err.msg);
          fflush(stdout); fprintf(stderr, "%s\n", p.err.msg.c_str()); exit(1);
        }
      }
    }
    n_regions = (long int)regs.size();
    R = n_regions > 0 ? new GenomicRegion *[n_regions] : NULL;
    for (long int k = 0; k < n_regions; k++) R[k] = regs[k];
  } else if (line) {
    n_regions = 1;
    cur_raw = line;
    R = new GenomicRegion *[1];
    R[0] = CreateRegion(line, src->line_no());
  }
  if (verbose) {
    std::cerr << "Reading from '" << (file == NULL ? "<standard input>" : file) << "'; ";
    std::cerr << "read-from-stdin = " << (from_stdin ? "true" : "false") << "; ";
    std::cerr << "load-in-memory = " << (load_in_memory ? "true" : "false") << "; ";
    std::cerr << "number of regions = " << n_regions << "; ";
    std::cerr << "format = " << format << "\n";
  }
  r_index = 0;
}

void GenomicRegionSet::Reset()
{
  if (from_stdin) PrintError("stdin cannot be reset!\n");
  if (file_ptr && !load_in_memory) { if (fseek(file_ptr, 0, SEEK_SET) != 0) PrintError("the stream cannot be reset!\n"); }
  if (load_in_memory) { r_index = 0; return; }
  if (R) { delete R[0]; delete[] R; R = NULL; }
  delete src; src = NULL;
  delete packed; packed = NULL;
  Init();
}

GenomicRegion *GenomicRegionSet::Get()
{
  if (n_regions == 0) return NULL;
  return !load_in_memory ? R[0] : (r_index >= n_regions ? NULL : R[r_index]);
}

GenomicRegion *GenomicRegionSet::PackedRegion(long int k)
{
  const gtxhost::GtxView &g = *packed;
  char line[512];
  const char strand = (g.minus[k >> 3] >> (k & 7)) & 1 ? '-' : '+';
  if (g.label) snprintf(line, sizeof line, "%s\t%ld\t%ld\t%ld\t0\t%c", g.chrom[g.chrom_idx[k]].c_str(), (long)g.start[k] - 1, (long)g.stop[k], (long)g.label[k], strand);
  else snprintf(line, sizeof line, "%s\t%ld\t%ld\t_\t0\t%c", g.chrom[g.chrom_idx[k]].c_str(), (long)g.start[k] - 1, (long)g.stop[k], strand);
  return new GenomicRegionBED(line, k + 1);
}

GenomicRegion *GenomicRegionSet::Next(bool retain_current)
{
  if (load_in_memory) { ++r_index; return r_index >= n_regions ? NULL : R[r_index]; }
  if (packed) {
    if (n_regions == 0) return NULL;
    if (r_index + 1 >= (long int)packed->n) return NULL;
    if (R[0] && !retain_current) delete R[0];
    R[0] = PackedRegion(++r_index);
    return R[0];
  }
  if (n_regions == 0 || !src) return NULL;
  char *line = src->Next();
  if (!line) return NULL;
  if (R[0] && !retain_current) delete R[0];
  cur_raw = line;
  R[0] = CreateRegion(line, src->line_no());
  return R[0];
}

GenomicRegion *GenomicRegionSet::Next(bool sorted_by_strand, bool retain_current)
{
  GenomicRegion *r0 = Get();
  if (r0 == NULL) return NULL;
  GenomicRegion *r = Next(true);
  if (r != NULL && r->IsBefore(r0, sorted_by_strand))
    r->PrintError(std::string("input regions are not sorted (sorted-by-strand = ") + (sorted_by_strand ? "true" : "false") + ")!");
  if (!load_in_memory) {
    if (!retain_current) delete r0;
    if (r == NULL) { R[0] = NULL; n_regions = 0; }            // end of the stream: Get() answers NULL from now on
  }
  return r;
}

const gtxhost::GtxView *GenomicRegionSet::DetachPacked(long int *current_record)
{
  if (load_in_memory || !packed) PrintError("[DetachPacked] not a streamed packed region file!");
  *current_record = n_regions > 0 ? r_index : (long int)packed->n;
  if (n_regions > 0) { delete R[0]; R[0] = NULL; }
  n_regions = 0;
  return packed;
}

long int GenomicRegionSet::StreamBytesLeft() { return (load_in_memory || !src) ? -1 : src->regular_file_bytes(); }

LineSource *GenomicRegionSet::DetachStream(std::string *current_line, long int *current_line_no)
{
  if (load_in_memory) PrintError("[DetachStream] the set is loaded in memory!");
  *current_line = n_regions > 0 ? cur_raw : std::string();
  *current_line_no = n_regions > 0 ? R[0]->n_line : 0;
  if (n_regions > 0) { delete R[0]; R[0] = NULL; }
  n_regions = 0;
  return src;
}

// ---------------------------------------------------------------------------------------------------
// GPU context shared by the classes of this file
// ---------------------------------------------------------------------------------------------------
// HIP start-up takes ~0.2 s: it runs on its own thread from the first region set on, next to the
// parsing of the reference file (GtxWarmUp), and is joined when the context is first needed.
// The classes of this file drive a gtx_group: one context per GPU (--ngpu N / GTX_NGPU, default 1; devices GTX_DEVICE,
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

// Page-locked batch buffers for the bulk packer (gtxhost::BatchArena): two of them, filled in turn by DrainSet -- the packer
// threads write the packed triples where the DMA engine reads them (gtx_host_alloc memory skips the library's staging copy, and
// the call returns with the copy in flight: the contract of include/gtx.h is "untouched until the NEXT call has returned", which
// two alternating buffers satisfy).  Made by the start-up thread behind the loading of the reference set.
static const size_t kBatchReads = getenv("GTX_HOST_BATCH_READS") && atol(getenv("GTX_HOST_BATCH_READS")) > 0 ? (size_t)atol(getenv("GTX_HOST_BATCH_READS")) : (8u << 20);   // reads per batch handed to the device
static const size_t kPoolBytes = (kBatchReads * 3 + (24u << 20)) * sizeof(int32_t);   // what BedPacker::NextBatch reserves for it
static struct { void *buf[2]; bool used[2]; gtx_ctx *owner; } g_pool = {{NULL, NULL}, {false, false}, NULL};
static std::future<void> g_pool_future;

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
void StdoutIsOurs()
{
  static bool checked = false;
  if (checked) return;
  checked = true;
  int n = g_ngpu;
  if (n <= 0) { const char *e = getenv("GTX_NGPU"); n = e ? atoi(e) : 1; }
  const char *f = getenv("GTX_GROUP_FORCE_RCCL"), *x = getenv("GTX_GROUP_SELF_EXCHANGE");
  if ((n > 1 || (f && atoi(f)) || (x && atoi(x))) && g_group_future.valid()) g_group_future.wait();
}

void GtxWarmUp()
{
  if (!g_group_future.valid()) {
    atexit(JoinStartUp);
    // (GTX_SYNC_STARTUP=1, diagnostic: bring the device up on the calling thread instead of next to the parsing of the index set)
    g_group_future = std::async(getenv("GTX_SYNC_STARTUP") ? std::launch::deferred : std::launch::async, CreateGroup);
  }
}

static gtx_group *Devices()
{
  static gtx_group *grp = NULL;
  if (!grp) {
    GtxWarmUp();
    grp = g_group_future.get();
    if (!grp) { fflush(stdout); fprintf(stderr, "\nError: %s\n", g_ctx_error.c_str()); exit(1); }
  }
  return grp;
}

static void CheckGrp(gtx_group *g, int rc)
{
  if (rc != GTX_OK) { fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, gtx_group_last_error(g)); exit(1); }
}

// Packs the rest of a query/input set batch by batch and hands every batch to `sink`, in order; `prep` (wait for the HIP context
// that the start-up thread is making, gtx_set_refs, *_begin) runs first.  In-memory sets are walked region by region with the same
// rules.  Two batches in turn, in the two page-locked buffers: one is packed while the device still reads the other (the hand-over
// returns with the copy in flight).  Measured and dropped: packing AHEAD of the hand-over on a helper thread, started before the HIP
// runtime is up -- batches outside the page-locked buffers cost first-touch page faults and a staging copy in the library, more
// page-locked memory to release at exit, and 100 M reads from text came out 10 % slower (0.95 -> 1.06 s on one box).
static std::atomic<bool> g_drain_stop(false);                 // set by a sink that has seen enough (an error it will raise after DrainSet): no more batches

// What DrainSet needs to have a streamed BED file tokenised on the device (gtx_count_add_text, include/gtx.h) instead of parsing it
// here: add(text, bytes, lines, rules) -> ticket, and needs_host(ticket).  The device takes the plain case only; a block with
// anything else in it comes back and is packed here, with the reference's reading of it and the reference's errors.
struct TextSink {
  std::function<bool()> usable;                                   // (asked behind prep(): one GPU)
  std::function<int(const char *, size_t, int64_t, const gtx_text_rules &, uint32_t)> add;   // (the last argument: GTX_TEXT_SAM, GTX_TEXT_GFF or 0, to go with the call's flags)
  std::function<bool(int)> needs_host;
};

static bool TextOnDevice(GenomicRegionSet *set, const PackOptions &opt, const TextSink *ts)
{
  static const char *e = getenv("GTX_TEXT_ON_DEVICE");        // 0: never; 1: whenever the input qualifies (tests); default: files of 32 MB or more
  if (!ts || (e && atoi(e) == 0)) return false;
  if (set->load_in_memory || (set->format != "BED" && set->format != "SAM" && set->format != "GFF")) return false;
  if (opt.guard || opt.collect_zero_length) return false;                 // (explode_blocks: a 12-column line sends its block back to the packer, which does it)
  if (!g_pool.buf[0] || !g_pool.buf[1] || !ts->usable()) return false;
  // a regular uncompressed file: worth it from 32 MB on.  A stream (stdin / a pipe, a .gz file, a FILE* of the caller's: -1) has no
  // size to go by: it takes the device path, and pump_text hands a first block that turns out to be all there is to the host packer
  const long left = set->StreamBytesLeft();
  return left < 0 || left >= ((e && atoi(e) == 1) ? 1 : (32l << 20));
}

// on_error (may be empty): called with the packer's error instead of dying with it, after the batch in hand -- which, under
// PackOptions::keep_prefix_on_error, holds the regions of the lines in front of the offending one -- has gone to `sink`; nothing more is packed
template <class Prep, class Sink>
static void DrainSet(GenomicRegionSet *set, PackOptions opt, Prep prep, Sink sink, const TextSink *text_sink = NULL,
                     const std::function<void(const PackError &)> &on_error = std::function<void(const PackError &)>())
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
    // blocks of complete lines straight into the two page-locked buffers, tokenised and counted on the device; what is not plain is
    // packed here.  Two blocks in flight: block i's verdict is collected before block i+2 is read over it.
    std::vector<const char *> names((size_t)opt.chroms->size());
    for (int i = 0; i < opt.chroms->size(); i++) names[i] = opt.chroms->name(i).c_str();
    gtx_text_rules rules;
    rules.chrom_names = names.empty() ? NULL : names.data(); rules.n_chrom = opt.chroms->size();
    rules.strand_aware = opt.strand_aware; rules.sorted_rules = opt.mode == gtxhost::PACK_OVERLAPS_SORTED || opt.mode == gtxhost::PACK_SCAN_SORTED; rules.sorted_by_strand = opt.sorted_by_strand;
    rules.max_label_value = opt.max_label_value;
    g_pool.used[0] = g_pool.used[1] = true;                      // (the buffers hold text now: a batch packed here takes heap memory)
    packer.UseTextBuffers((char *)g_pool.buf[0], (char *)g_pool.buf[1], kPoolBytes);
    PackedBatch batch;
    if (!packer.PackPrimedText(&batch, &err) && !on_error) DiePack(err);
    if (worth(batch)) sink(batch);
    if (err.set) { on_error(err); g_drain_stop = true; g_pool.used[0] = g_pool.used[1] = false; return; }
    BedPacker::TextBlock blk[2]; int ticket[2] = {-1, -1}; bool host_only = false, first_block = true;
    static const bool text_forced = getenv("GTX_TEXT_ON_DEVICE") && atoi(getenv("GTX_TEXT_ON_DEVICE")) == 1;
    long on_device = 0, redone = 0, host_blocks = 0;
    auto settle = [&](int k) {                                   // the verdict on the block in blk[k]
      if (ticket[k] < 0) return;
      const bool redo = text_sink->needs_host(ticket[k]);
      ticket[k] = -1;
      if (!redo) { on_device++; return; }
      redone++;
      batch.clear();
      const bool ok = packer.PackTextBlock(blk[k], &batch, &err);
      if (err.set && !on_error) DiePack(err);
      (void)ok;
      if (worth(batch)) sink(batch);
      if (err.set) { on_error(err); g_drain_stop = true; }
    };
    for (int cur = 0;; cur ^= 1) {
      settle(cur);                                               // (its buffer is about to be read over)
      if (g_drain_stop) break;
      if (!packer.NextTextBlock(&blk[cur])) break;
      BedPacker::TextBlock &b = blk[cur];
      if (!b.seam_ok) host_only = true;                          // a last line that could not be read: no seam key for the device
      if (first_block && !text_forced && b.bytes < (32u << 20) && packer.SourceAtEnd()) host_only = true;   // a short stream: the host packer is done before the device has the text
      first_block = false;
      if (host_only) {
        host_blocks++;
        batch.clear();
        packer.PackTextBlock(b, &batch, &err);
        if (err.set && !on_error) { settle(cur ^ 1); DiePack(err); }
        if (worth(batch)) sink(batch);
        if (err.set) { on_error(err); g_drain_stop = true; break; }
        continue;
      }
      rules.have_prev = b.have_prev; rules.prev_chrom = b.prev_chrom.c_str(); rules.prev_strand = b.prev_strand; rules.prev_start = b.prev_start;
      ticket[cur] = text_sink->add(b.text, b.bytes, b.n_lines, rules, opt.sam ? GTX_TEXT_SAM : opt.gff ? GTX_TEXT_GFF : 0u);
      if (on_error) settle(cur);                                 // (a caller that goes on after an error wants nothing behind the offending line counted: one block at a time)
    }
    settle(0); settle(1);
    if (getenv("GTX_TEXT_TRACE")) fprintf(stderr, "[gtx text] blocks tokenised on the device: %ld, sent back to the host packer: %ld, packed on the host from the start: %ld\n", on_device, redone, host_blocks);
    g_pool.used[0] = g_pool.used[1] = false;
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

// quick order hint for the kernel choice (a wrong hint only costs speed): sample adjacent pairs
static bool LooksSorted(const gtxhost::RawVec &tri)
{
  const size_t n = tri.size() / 3;
  if (n < 2) return true;
  const size_t stride = n > 4096 ? n / 4096 : 1;
  int descents = 0;                                     // a batch is a few sorted runs at most (e.g. the '+' then the '-' reads)
  for (size_t i = 0; i + 1 < n; i += stride) {
    const int32_t *a = &tri[3 * i], *b = a + 3;
    if ((b[0] < a[0] || (b[0] == a[0] && b[1] < a[1])) && ++descents > 2) return false;
  }
  return true;
}

// the same hint from the text of a block: pairs of adjacent lines at ~4096 places, (chromosome token, start column) compared.
// format: GTX_TEXT_SAM, GTX_TEXT_GFF or 0 for BED
static bool TextLooksSorted(const char *text, size_t bytes, uint32_t format = 0)
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

// an error of a member context, reported through the group's channel (CheckGrp prints gtx_group_last_error)

static bool LooksSortedVec(const std::vector<int32_t> &tri)
{
  const size_t n = tri.size() / 3;
  if (n < 2) return true;
  const size_t stride = n > 4096 ? n / 4096 : 1;
  for (size_t i = 0; i + 1 < n; i += stride) {
    const int32_t *a = &tri[3 * i], *b = a + 3;
    if (b[0] < a[0] || (b[0] == a[0] && b[1] < a[1])) return false;
  }
  return true;                                            // (a hint: the device verifies it and falls back by itself)
}

// ---------------------------------------------------------------------------------------------------
// GenomicRegionSetOverlaps
// ---------------------------------------------------------------------------------------------------
GenomicRegionSetOverlaps::GenomicRegionSetOverlaps(GenomicRegionSet *QuerySet, GenomicRegionSet *IndexSet)
{
  this->QuerySet = QuerySet; this->IndexSet = IndexSet; current_qreg = NULL; current_ireg = NULL;
}

GenomicRegionSetOverlaps::~GenomicRegionSetOverlaps() {}

unsigned long int *GenomicRegionSetOverlaps::CountIndexOverlaps(bool match_gaps, bool ignore_strand, long int max_label_value)
{
  // single-interval regions have no gaps: both settings select the same pairs (genomic_intervals.cpp:5226)
  if (IndexSet->load_in_memory == false) {
    fprintf(stderr, "[GenomicRegionSetOverlaps::CountIndexOverlaps]: index set must be loaded in memory for this operation!\n");
    exit(1);
  }
  return Reduce(false, match_gaps, ignore_strand, max_label_value);
}

unsigned long int *GenomicRegionSetOverlaps::CalcIndexCoverage(bool match_gaps, bool ignore_strand, long int max_label_value)
{
  // single intervals: the envelope formula (:5278) and CalcOverlap (:1196-1202) coincide except that the former is not clamped
  // at 0 -- pairs with an inverted interval under the sorted merge (GTX_GAPS_FORMULA)
  if (IndexSet->load_in_memory == false) {
    fprintf(stderr, "[GenomicRegionSetOverlaps::CalcIndexCoverage]: index set must be loaded in memory for this operation!\n");
    exit(1);
  }
  return Reduce(true, match_gaps, ignore_strand, max_label_value);
}

unsigned long int *GenomicRegionSetOverlaps::Reduce(bool coverage, bool match_gaps, bool ignore_strand, long int max_label_value)
{
  const long int M = IndexSet->n_regions;
  const SortedGenomicRegionSetOverlaps *merge = dynamic_cast<const SortedGenomicRegionSetOverlaps *>(this);
  const bool sorted = merge != NULL, by_strand = merge && merge->sorted_by_strand;
  if (!ignore_strand) CheckGffStrands(IndexSet);
  for (long int k = 0; k < M; k++) IndexSet->R[k]->n_line = k;                       // :5309
  Mark("CountIndexOverlaps: start");

  // ---- index side ----
  // Sorted merge: the reference notices an index set that is out of order only at the moment the merge pulls the offending
  // region (genomic_intervals.cpp:5868).  v = the first such region; the regions from v on are never matched (either the
  // queries end before the merge gets there, or the run ends with the error), the packer's IndexGuard decides which.
  long int v = M;
  if (sorted) for (long int k = 1; k < M; k++) if (IndexSet->R[k]->IsBefore(IndexSet->R[k - 1], by_strand)) { v = k; break; }
  gtxhost::IndexGuard guard;
  if (v < M) {
    guard.by_strand = by_strand;
    for (long int k = 0; k < v; k++) {
      GenomicInterval *i = IndexSet->R[k]->I.front();
      guard.chrom.push_back(i->CHROMOSOME); guard.strand.push_back(i->STRAND); guard.start.push_back(i->START); guard.stop.push_back(IndexSet->R[k]->I.back()->STOP);
    }
    char buf[160];
    snprintf(buf, sizeof buf, "\nError: Line %ld: index regions are not sorted (sorted-by-strand = %s)!", v, by_strand ? "true" : "false");
    guard.msg = buf;
  }
  ChromTable chroms;
  bool explode = false;                                                             // coverage without -gaps over multi-interval index regions
  bool blocks_mode = false;                                                         // count without -gaps over multi-interval index regions
  const char *last_name = NULL;                                                     // region files repeat a chromosome many times in a row
  for (long int k = 0; k < v; k++) {
    GenomicRegion *r = IndexSet->R[k];
    GenomicInterval *i = r->I.front();
    if (r->I.size() > 1) {
      // a multi-interval (BED12) region: with -gaps it is matched on its envelope (:5226, :5752, :5278) -- what the device computes.
      // Without: coverage is a sum over ALL interval pairs of the two regions (CalcOverlap :1196-1202, pairs that do not overlap
      // add 0), so the intervals go to the device one by one (`explode`) and a region's value is the sum of its intervals';
      // count needs "some interval pair overlaps" (:1167-1172), which no sum of independent pieces gives: the device counts on the
      // envelopes and settles the pairs with a multi-interval side one by one (`blocks_mode`, gtx_set_ref_blocks);
      if (!r->IsCompatibleSortedAndNonoverlapping()) r->PrintError("index regions should be compatible, sorted and non-overlapping!");   // :5607, :5853
      if (!match_gaps && coverage) explode = true;
      if (!match_gaps && !coverage) blocks_mode = true;
    }
    if (!sorted && (i->START > r->I.back()->STOP || r->I.back()->STOP <= 0)) continue;   // :5609, :5659
    if (last_name && strcmp(last_name, i->CHROMOSOME) == 0) continue;
    chroms.Add(i->CHROMOSOME); last_name = i->CHROMOSOME;
  }
  chroms.Freeze();
  const int n_chrom = chroms.size();
  const bool strand_aware = !ignore_strand;
  bool zero_length_refs = false;
  std::vector<int32_t> refs((size_t)3 * (M > 0 ? M : 1));
  last_name = NULL; int last_id = -1;
  for (long int k = 0; k < M; k++) {
    GenomicRegion *r = IndexSet->R[k];
    GenomicInterval *i = r->I.front();
    if (k >= v) { refs[3 * k] = -1; refs[3 * k + 1] = 1; refs[3 * k + 2] = 0; continue; }   // behind the out-of-order spot: a placeholder
    const long int STOP = r->I.back()->STOP;                                       // the envelope's end (single interval: its own)
    if (sorted && i->START == STOP + 1) zero_length_refs = true;
    if (i->START >= INT_MAX - 1 || STOP >= INT_MAX - 1 || i->START <= INT_MIN + 1 || STOP <= INT_MIN + 1)
      r->PrintError("coordinate does not fit the packed 32-bit representation of the MI355X path!");
    if (!last_name || strcmp(last_name, i->CHROMOSOME) != 0) { last_name = i->CHROMOSOME; last_id = chroms.Find(i->CHROMOSOME); }
    const int id = last_id;
    if (id < 0) { refs[3 * k] = -1; refs[3 * k + 1] = 1; refs[3 * k + 2] = 0; continue; }  // invalid region: never matches
    refs[3 * k] = id + ((strand_aware && i->STRAND == '-') ? n_chrom : 0);
    refs[3 * k + 1] = (int32_t)i->START; refs[3 * k + 2] = (int32_t)STOP;
  }
  // `explode`: one device region per interval; first_piece[k] .. first_piece[k+1] are region k's
  std::vector<long int> first_piece;
  long int MD = M;
  if (explode) {
    std::vector<int32_t> pieces;
    first_piece.assign((size_t)M + 1, 0);
    for (long int k = 0; k < M; k++) {
      first_piece[k] = (long int)(pieces.size() / 3);
      GenomicRegion *r = IndexSet->R[k];
      if (refs[3 * k] < 0 || r->I.size() == 1) { pieces.insert(pieces.end(), refs.begin() + 3 * k, refs.begin() + 3 * k + 3); continue; }
      for (GenomicIntervalSet::iterator b = r->I.begin(); b != r->I.end(); b++) {
        if ((*b)->START >= INT_MAX - 1 || (*b)->STOP >= INT_MAX - 1 || (*b)->START <= INT_MIN + 1 || (*b)->STOP <= INT_MIN + 1)
          r->PrintError("coordinate does not fit the packed 32-bit representation of the MI355X path!");
        pieces.push_back(refs[3 * k]); pieces.push_back((int32_t)(*b)->START); pieces.push_back((int32_t)(*b)->STOP);
      }
    }
    first_piece[M] = (long int)(pieces.size() / 3);
    MD = first_piece[M];
    refs.swap(pieces);
  }
  // `blocks_mode`: the intervals of every region, as gtx_set_ref_blocks takes them
  std::vector<int64_t> blk_first; std::vector<int32_t> blk_iv;
  if (blocks_mode) {
    blk_first.assign((size_t)M + 1, 0);
    for (long int k = 0; k < M; k++) {
      blk_first[k] = (int64_t)(blk_iv.size() / 2);
      GenomicRegion *r = IndexSet->R[k];
      if (refs[3 * k] < 0 || r->I.size() == 1) { blk_iv.push_back(refs[3 * k + 1]); blk_iv.push_back(refs[3 * k + 2]); continue; }
      long int prev_stop = LONG_MIN;
      for (GenomicIntervalSet::iterator b = r->I.begin(); b != r->I.end(); b++) {
        if ((*b)->START >= INT_MAX - 1 || (*b)->STOP >= INT_MAX - 1 || (*b)->START <= INT_MIN + 1 || (*b)->STOP <= INT_MIN + 1)
          r->PrintError("coordinate does not fit the packed 32-bit representation of the MI355X path!");
        if ((*b)->STOP < prev_stop) r->PrintError("multi-interval (BED12) region with an interval of negative size is outside the MI355X counting path!");
        prev_stop = (*b)->STOP;
        blk_iv.push_back((int32_t)(*b)->START); blk_iv.push_back((int32_t)(*b)->STOP);
      }
    }
    blk_first[M] = (int64_t)(blk_iv.size() / 2);
  }
  Mark("index packed");
  gtx_group *grp = NULL;
  const int n_classes = std::max(1, n_chrom * (strand_aware ? 2 : 1));
  auto device_side = [&](bool cover) {                              // (on DrainSet's hand-over thread, while the queries are already being packed)
    grp = Devices();
    Mark("device ready");
    CheckGrp(grp, gtx_group_set_refs(grp, refs.data(), MD, n_classes, sorted ? GTX_REFS_KEEP_ZERO_LENGTH : 0));
    if (blocks_mode) CheckGrp(grp, gtx_group_set_ref_blocks(grp, blk_first.data(), blk_iv.data()));
    Mark("gtx_set_refs done");
    CheckGrp(grp, cover ? gtx_group_coverage_begin(grp) : gtx_group_count_begin(grp));
  };

  // ---- query side: stream -> packed batches -> device ----
  PackOptions opt;
  opt.mode = sorted ? gtxhost::PACK_OVERLAPS_SORTED : gtxhost::PACK_OVERLAPS_UNSORTED;
  opt.chroms = &chroms; opt.strand_aware = strand_aware; opt.sorted_by_strand = by_strand;
  opt.max_label_value = max_label_value; opt.collect_zero_length = !coverage && sorted && zero_length_refs;
  opt.match_gaps = match_gaps;
  opt.explode_blocks = coverage && !match_gaps;                  // multi-interval queries: their intervals one by one (see the index side)
  opt.collect_blocks = !coverage && !match_gaps;                 // ... or on a list of their own, for the pair kernel
  if (v < M) opt.guard = &guard;
  std::vector<int32_t> zero_len;
  unsigned long int *hits = new unsigned long int[M > 0 ? M : 1];
  gtx_count_info info;
  // the query file's text tokenised on the device where that applies (one GPU, a plain BED file: TextOnDevice)
  TextSink text_sink;
  text_sink.usable = [&] { return gtx_group_size(grp) >= 1; };     // (several GPUs: the blocks go to the members in turn, gtx_group_count_add_text)
  text_sink.needs_host = [&](int ticket) { int redo = 0; CheckGrp(grp, gtx_group_text_result(grp, ticket, &redo)); return redo != 0; };
  if (coverage) {
    // zero-length reads (sorted rules let them through) and zero-length regions contribute 0: the device leaves them out
    const uint32_t cflags = sorted ? (GTX_ZERO_LENGTH_OK | (match_gaps ? GTX_GAPS_FORMULA : 0u)) : 0u;
    text_sink.add = [&](const char *text, size_t bytes, int64_t lines, const gtx_text_rules &rules, uint32_t text_flags) {
      int ticket = -1;
      CheckGrp(grp, gtx_group_coverage_add_text(grp, text, bytes, lines, &rules, cflags | text_flags | (sorted ? GTX_READS_SORTED : 0u), &ticket));
      return ticket;
    };
    DrainSet(QuerySet, opt, [&] { device_side(true); }, [&](const PackedBatch &b) {
      CheckGrp(grp, gtx_group_coverage_add(grp, b.tri.data(), b.w.empty() ? NULL : b.w.data(), (int64_t)(b.tri.size() / 3), cflags));
    }, &text_sink);
    Mark("queries packed and enqueued");
    if (explode) {
      std::vector<uint64_t> part((size_t)std::max<long int>(MD, 1));
      CheckGrp(grp, gtx_group_coverage_end(grp, part.data(), &info));
      for (long int k = 0; k < M; k++) { unsigned long int sum = 0; for (long int j = first_piece[k]; j < first_piece[k + 1]; j++) sum += part[j]; hits[k] = sum; }
    } else
    CheckGrp(grp, gtx_group_coverage_end(grp, (uint64_t *)hits, &info));
    if (info.n_unplaced != 0) { fflush(stdout); fprintf(stderr, "\nError: %ld inverted query regions (start > stop) exceed what the MI355X path sets aside for pairwise matching!\n", (long)info.n_unplaced); exit(1); }
    Mark("coverage on the host");
    return hits;
  }
  const uint32_t mode_flags = sorted ? GTX_ZERO_LENGTH_OK : 0;
  text_sink.add = [&](const char *text, size_t bytes, int64_t lines, const gtx_text_rules &rules, uint32_t text_flags) {
    int ticket = -1;
    // (the sorted merge's input is in order, or the block comes back; the bin index takes any order: a look at the text decides the kernel)
    const uint32_t flags = mode_flags | text_flags | ((sorted || TextLooksSorted(text, bytes, text_flags & (GTX_TEXT_SAM | GTX_TEXT_GFF))) ? GTX_READS_SORTED : 0);
    CheckGrp(grp, gtx_group_count_add_text(grp, text, bytes, lines, &rules, flags, &ticket));
    return ticket;
  };
  DrainSet(QuerySet, opt, [&] { device_side(false); }, [&](const PackedBatch &b) {
    uint32_t flags = mode_flags | (LooksSorted(b.tri) ? GTX_READS_SORTED : 0);
    CheckGrp(grp, gtx_group_count_add(grp, b.tri.data(), b.w.empty() ? NULL : b.w.data(), (int64_t)(b.tri.size() / 3), flags));
    if (!b.m_cnt.empty()) {                                       // the multi-interval queries of the batch
      std::vector<int64_t> first(b.m_cnt.size() + 1, 0);
      for (size_t i = 0; i < b.m_cnt.size(); i++) first[i + 1] = first[i] + b.m_cnt[i];
      CheckGrp(grp, gtx_group_count_add_regions(grp, b.m_tri.data(), b.m_w.data(), first.data(), b.m_blocks.data(), (int64_t)b.m_cnt.size()));
    }
    zero_len.insert(zero_len.end(), b.zero_len.begin(), b.zero_len.end());
  }, &text_sink);
  Mark("queries packed and enqueued");
  CheckGrp(grp, gtx_group_count_end(grp, (uint64_t *)hits, &info));
  if (getenv("GTX_TIMING") && gtx_group_size(grp) > 1) {
    std::vector<int64_t> mr((size_t)gtx_group_size(grp));
    gtx_group_member_reads(grp, mr.data());
    for (size_t i = 0; i < mr.size(); i++) fprintf(stderr, "[gtx] GPU %zu counted %ld reads\n", i, (long)mr[i]);
  }
  Mark("counts on the host");
  // (sorted merge: n_degenerate counts the inverted reads, which the library matched pair by pair)
  if (!sorted && info.n_degenerate != 0) { fflush(stdout); fprintf(stderr, "\nError: internal: the packer let %ld degenerate reads through\n", (long)info.n_degenerate); exit(1); }
  if (info.n_unplaced != 0) { fflush(stdout); fprintf(stderr, "\nError: %ld inverted query regions (start > stop) exceed what the MI355X path sets aside for pairwise matching!\n", (long)info.n_unplaced); exit(1); }

  // sorted merge only: a zero-length read never overlaps a zero-length region at the same spot
  // (rS <= qE and rE >= qS cannot both hold), while the rank difference counts it as -1: undo that.
  if (!zero_len.empty()) {
    for (long int k = 0; k < M; k++) {
      if (refs[3 * k + 1] != refs[3 * k + 2] + 1) continue;
      for (size_t z = 0; z + 2 < zero_len.size(); z += 3)
        if (zero_len[z] == refs[3 * k] && zero_len[z + 1] == refs[3 * k + 1]) hits[k] += (unsigned long int)(long int)zero_len[z + 2];
    }
  }
  return hits;
}

// ---- per-query iteration (host side, like the reference's: these calls hand out GenomicRegion pointers) -------------------
// What GetMatch/NextMatch deliver are candidates on the envelopes; the filter of genomic_intervals.cpp:5224-5248 decides which of them
// are overlaps: under match_gaps the envelope is all that counts, otherwise some interval pair must overlap; and unless strands are
// ignored both regions must lie on the same strand (that of their first interval).
namespace {
struct OverlapFilter {
  GenomicRegion *query; bool gaps, any_strand;
  bool operator()(GenomicRegion *cand) const
  {
    if (!any_strand && query->I.front()->STRAND != cand->I.front()->STRAND) return false;
    return gaps || query->OverlapsWith(cand, any_strand);
  }
};

// value(r) summed over the overlaps of the current query, in `unsigned long` like the reference's accumulators (:5254-5263, :5291-5296)
template <class Value>
unsigned long int sum_over_overlaps(GenomicRegionSetOverlaps *o, bool match_gaps, bool ignore_strand, Value value)
{
  unsigned long int total = 0;
  GenomicRegion *r = o->GetOverlap(match_gaps, ignore_strand);
  while (r != NULL) { total += (unsigned long int)value(r); r = o->NextOverlap(match_gaps, ignore_strand); }
  return total;
}
}  // namespace

GenomicRegion *GenomicRegionSetOverlaps::GetOverlap(bool match_gaps, bool ignore_strand)
{
  const OverlapFilter overlaps = {current_qreg, match_gaps, ignore_strand};
  GenomicRegion *cand = GetMatch();
  while (cand != NULL && !overlaps(cand)) cand = NextMatch();
  return cand;
}

GenomicRegion *GenomicRegionSetOverlaps::NextOverlap(bool match_gaps, bool ignore_strand)
{
  const OverlapFilter overlaps = {current_qreg, match_gaps, ignore_strand};
  GenomicRegion *cand = NextMatch();
  while (cand != NULL && !overlaps(cand)) cand = NextMatch();
  return cand;
}

unsigned long int GenomicRegionSetOverlaps::CalcQueryCoverage(bool match_gaps, bool ignore_strand, long int max_label_value)
{
  GenomicRegion *q = current_qreg;
  return sum_over_overlaps(this, match_gaps, ignore_strand, [=](GenomicRegion *r) -> long int {
    // envelope against envelope under match_gaps (not clamped: :5258), interval pairs otherwise; times the INDEX region's label value
    const long int len = match_gaps ? std::min(r->I.back()->STOP, q->I.back()->STOP) - std::max(r->I.front()->START, q->I.front()->START) + 1
                                    : q->CalcOverlap(r, ignore_strand);
    return len * r->GetLabelValue(max_label_value);
  });
}

unsigned long int GenomicRegionSetOverlaps::CountQueryOverlaps(bool match_gaps, bool ignore_strand, long int max_label_value)
{
  return sum_over_overlaps(this, match_gaps, ignore_strand, [=](GenomicRegion *r) -> long int { return r->GetLabelValue(max_label_value); });
}

// The bin index of UnsortedGenomicRegionSetOverlaps (genomic_intervals.cpp:5593-5675) for GetMatch/NextMatch: a region lives at the
// lowest level where its (clamped) start and its stop fall into one bin; a bin keeps its regions in the order they came.
struct UnsortedGenomicRegionSetOverlaps::MatchIndex {
  std::vector<int> bits;
  struct Chrom { std::vector<long int> n_bins; std::vector<std::vector<std::vector<long int> > > bins; };   // [level][bin] -> region ordinals
  std::map<std::string, Chrom> chrom;
  // cursor of the walk for the current query (:5729-5764)
  Chrom *cur; long int start, stop, b, b_stop; int l; long int at;          // `at` counts down inside the bin: last inserted first
};

UnsortedGenomicRegionSetOverlaps::UnsortedGenomicRegionSetOverlaps(GenomicRegionSet *QuerySet, GenomicRegionSet *IndexSet, const char *bin_bits)
    : GenomicRegionSetOverlaps(QuerySet, IndexSet)
{
  // -B tunes the reference's bin index; the rank structure on the device has no bins, the host-side iteration (GetMatch) does
  match = NULL; bin_bits_ = bin_bits ? bin_bits : "";
  if (IndexSet->load_in_memory == false) { fprintf(stderr, "Error: [UnsortedGenomicRegionSetOverlaps] index regions must be loaded in memory!\n"); exit(1); }
}
UnsortedGenomicRegionSetOverlaps::~UnsortedGenomicRegionSetOverlaps() { delete match; }
GenomicRegion *UnsortedGenomicRegionSetOverlaps::GetQuery()
{
  current_qreg = QuerySet->Get();
  if (current_qreg && !current_qreg->IsCompatibleSortedAndNonoverlapping()) current_qreg->PrintError("query regions should be compatible, sorted and non-overlapping!");
  return current_qreg;
}
GenomicRegion *UnsortedGenomicRegionSetOverlaps::NextQuery()
{
  current_qreg = QuerySet->Next();
  if (current_qreg && !current_qreg->IsCompatibleSortedAndNonoverlapping()) current_qreg->PrintError("query regions should be compatible, sorted and non-overlapping!");
  return current_qreg;
}

GenomicRegion *UnsortedGenomicRegionSetOverlaps::GetMatch()
{
  if (!match) {
    match = new MatchIndex;
    MatchIndex &mx = *match;
    // levels: the listed shift widths, the last one forced to 60 bits = one bin (:5619-5636)
    if (bin_bits_.empty()) mx.bits = {17, 20, 23, 26, 60};
    else {
      size_t p = 0;
      for (;;) { size_t q = bin_bits_.find(',', p); mx.bits.push_back(atoi(bin_bits_.substr(p, q == std::string::npos ? q : q - p).c_str())); if (q == std::string::npos) break; p = q + 1; }
      mx.bits.push_back(60);
    }
    const int L = (int)mx.bits.size();
    std::map<std::string, long int> chrom_size;
    for (long int k = 0; k < IndexSet->n_regions; k++) {
      GenomicRegion *r = IndexSet->R[k];
      if (!r->IsCompatibleSortedAndNonoverlapping()) r->PrintError("index regions should be compatible, sorted and non-overlapping!");
      const long int start = r->I.front()->START, stop = r->I.back()->STOP;
      if (start > stop || stop <= 0) continue;
      std::map<std::string, long int>::iterator it = chrom_size.find(r->I.front()->CHROMOSOME);
      if (it == chrom_size.end()) chrom_size[r->I.front()->CHROMOSOME] = stop; else it->second = std::max(it->second, stop);
    }
    for (std::map<std::string, long int>::iterator it = chrom_size.begin(); it != chrom_size.end(); it++) {
      MatchIndex::Chrom &c = mx.chrom[it->first];
      c.n_bins.resize(L); c.bins.resize(L);
      for (int l = 0; l < L; l++) { c.n_bins[l] = (it->second >> mx.bits[l]) + 1; c.bins[l].resize((size_t)c.n_bins[l]); }
    }
    for (long int k = 0; k < IndexSet->n_regions; k++) {
      GenomicRegion *r = IndexSet->R[k];
      long int start = r->I.front()->START; const long int stop = r->I.back()->STOP;
      if (start > stop || stop <= 0) continue;                                     // :5659
      if (start <= 0) start = 1;
      MatchIndex::Chrom &c = mx.chrom[r->I.front()->CHROMOSOME];
      for (int l = 0; l < L; l++) if ((start >> mx.bits[l]) == (stop >> mx.bits[l])) { c.bins[l][(size_t)(start >> mx.bits[l])].push_back(k); break; }
    }
  }
  MatchIndex &mx = *match;
  std::map<std::string, MatchIndex::Chrom>::iterator it = mx.chrom.find(current_qreg->I.front()->CHROMOSOME);
  mx.cur = it == mx.chrom.end() ? NULL : &it->second;
  if (mx.cur == NULL) return current_ireg = NULL;
  mx.l = 0;
  mx.start = current_qreg->I.front()->START; mx.stop = current_qreg->I.back()->STOP;
  if (mx.stop <= 0) current_qreg->PrintError("stop position must be positive!");
  if (mx.start > mx.stop) current_qreg->PrintError("start position cannot be greater than stop position!");
  if (mx.start <= 0) mx.start = 1;
  mx.b = mx.start >> mx.bits[0];
  mx.b_stop = std::min(mx.stop >> mx.bits[0], mx.cur->n_bins[0] - 1);
  if (mx.b >= mx.cur->n_bins[0]) { mx.cur = NULL; return current_ireg = NULL; }
  mx.at = (long int)mx.cur->bins[0][(size_t)mx.b].size();
  return NextMatch();
}

GenomicRegion *UnsortedGenomicRegionSetOverlaps::NextMatch()
{
  if (!match || match->cur == NULL) return current_ireg = NULL;
  MatchIndex &mx = *match;
  const int L = (int)mx.bits.size();
  for (;;) {
    if (mx.l < L && mx.b <= mx.b_stop && mx.b < mx.cur->n_bins[mx.l]) {
      const std::vector<long int> &bin = mx.cur->bins[mx.l][(size_t)mx.b];
      while (mx.at > 0) {
        GenomicRegion *r = IndexSet->R[bin[(size_t)--mx.at]];
        if (mx.start <= r->I.back()->STOP && mx.stop >= r->I.front()->START) return current_ireg = r;
      }
    }
    mx.b++;
    if (mx.l >= L || mx.b > mx.b_stop) {
      mx.l++;
      if (mx.l >= L) break;
      mx.b = mx.start >> mx.bits[mx.l];
      mx.b_stop = std::min(mx.stop >> mx.bits[mx.l], mx.cur->n_bins[mx.l] - 1);
    }
    mx.at = (mx.b <= mx.b_stop && mx.b < mx.cur->n_bins[mx.l]) ? (long int)mx.cur->bins[mx.l][(size_t)mx.b].size() : 0;
  }
  mx.cur = NULL;
  return current_ireg = NULL;
}
bool UnsortedGenomicRegionSetOverlaps::Done() { return current_qreg == NULL; }

SortedGenomicRegionSetOverlaps::SortedGenomicRegionSetOverlaps(GenomicRegionSet *QuerySet, GenomicRegionSet *IndexSet, bool sorted_by_strand)
    : GenomicRegionSetOverlaps(QuerySet, IndexSet)
{
  this->sorted_by_strand = sorted_by_strand;
  buffer_at_ = 0; index_at_ = 0; have_union_ = false; union_strand_ = '+'; union_start_ = union_stop_ = 0;
  current_qreg = QuerySet->Get();
  current_ireg = IndexSet->Get();
}
SortedGenomicRegionSetOverlaps::~SortedGenomicRegionSetOverlaps() {}

// LoadIndexBuffer (genomic_intervals.cpp:5844-5873): drop the buffer when the query has passed its union interval, then pull index
// regions while the query is not before them, keeping the ones it meets; the order of the index set is checked as it is pulled
void SortedGenomicRegionSetOverlaps::LoadIndexBuffer()
{
  if (current_qreg == NULL) return;
  if (!IndexSet->load_in_memory) { fprintf(stderr, "Error: [SortedGenomicRegionSetOverlaps] per-query iteration needs the index set loaded in memory in this build!\n"); exit(1); }
  if (!buffer_.empty() && have_union_) {
    GenomicInterval u(union_chrom_.c_str(), union_strand_, union_start_, union_stop_);
    GenomicInterval q(current_qreg->I.front()->CHROMOSOME, current_qreg->I.front()->STRAND, current_qreg->I.front()->START, current_qreg->I.back()->STOP);
    if (q.CalcDirection(&u, sorted_by_strand) > 0) { buffer_.clear(); have_union_ = false; }
  }
  while (index_at_ < IndexSet->n_regions) {
    GenomicRegion *r = IndexSet->R[index_at_];
    if (!r->IsCompatibleSortedAndNonoverlapping()) r->PrintError("index regions should be compatible, sorted and non-overlapping!");
    const int d = current_qreg->CalcDirection(r, sorted_by_strand);
    if (d < 0) break;
    if (d == 0) {
      if (buffer_.empty()) { union_chrom_ = r->I.front()->CHROMOSOME; union_strand_ = r->I.front()->STRAND; union_start_ = r->I.front()->START; union_stop_ = r->I.back()->STOP; have_union_ = true; }
      else { union_start_ = std::min(union_start_, r->I.front()->START); union_stop_ = std::max(union_stop_, r->I.back()->STOP); }
      buffer_.push_back(index_at_);
    }
    index_at_++;
    if (index_at_ < IndexSet->n_regions && IndexSet->R[index_at_]->IsBefore(r, sorted_by_strand))
      IndexSet->R[index_at_]->PrintError(std::string("index regions are not sorted (sorted-by-strand = ") + (sorted_by_strand ? "true" : "false") + ")!");
  }
  buffer_at_ = 0;
  current_ireg = buffer_.empty() ? NULL : IndexSet->R[buffer_[0]];
}

GenomicRegion *SortedGenomicRegionSetOverlaps::GetQuery()
{
  current_qreg = QuerySet->Get();
  if (current_qreg && !current_qreg->IsCompatibleSortedAndNonoverlapping()) current_qreg->PrintError("query regions should be compatible, sorted and non-overlapping!");
  LoadIndexBuffer();
  return current_qreg;
}
GenomicRegion *SortedGenomicRegionSetOverlaps::NextQuery()
{
  GenomicRegion *prev = QuerySet->Get();
  GenomicRegion *next = QuerySet->Next(true);
  if (next != NULL && !next->IsCompatibleSortedAndNonoverlapping()) next->PrintError("query regions should be compatible, sorted and non-overlapping!");
  if (next != NULL && prev != NULL && next->IsBefore(prev, sorted_by_strand))
    next->PrintError(std::string("query regions are not sorted (sorted-by-strand = ") + (sorted_by_strand ? "true" : "false") + ")!");
  if (!QuerySet->load_in_memory && next != NULL) delete prev;
  current_qreg = next;
  LoadIndexBuffer();
  return current_qreg;
}
// :5903-5918: buffered regions the query has passed are dropped, the first one ahead of it ends the walk
GenomicRegion *SortedGenomicRegionSetOverlaps::GetMatch()
{
  if (current_qreg == NULL || current_ireg == NULL) return NULL;
  for (;;) {
    const int d = current_qreg->CalcDirection(current_ireg, sorted_by_strand);
    if (d > 0) {
      buffer_.erase(buffer_.begin() + (long)buffer_at_);
      if (buffer_at_ >= buffer_.size()) return current_ireg = NULL;
      current_ireg = IndexSet->R[buffer_[buffer_at_]];
    } else if (d < 0) return NULL;
    else return current_ireg;
  }
}
GenomicRegion *SortedGenomicRegionSetOverlaps::NextMatch()
{
  buffer_at_++;
  current_ireg = buffer_at_ >= buffer_.size() ? NULL : IndexSet->R[buffer_[buffer_at_]];
  if (current_ireg == NULL) return NULL;
  return GetMatch();
}
bool SortedGenomicRegionSetOverlaps::Done() { return current_qreg == NULL || (index_at_ >= IndexSet->n_regions && buffer_.empty()); }

// ---------------------------------------------------------------------------------------------------
// scanners
// ---------------------------------------------------------------------------------------------------
static int g_keep_next = -1;                                      // KeepNextOnDevice: the slot the next scanner keeps its windows in

GenomicRegionSetScanner::GenomicRegionSetScanner(GenomicRegionSet *R, StringLIntMap *bounds, long int win_step, long int win_size,
                                                 long int max_label_value, bool ignore_strand, char preprocess)
{
  if (R->format == "SEQ") { std::cerr << "Error: this operation does not accept SEQ format!\n"; exit(1); }
  if (bounds == NULL) { std::cerr << "Error: this operation requires genomic bounds!\n"; exit(1); }
  this->R = R; this->bounds = bounds; this->win_step = win_step; this->win_size = win_size;
  this->max_label_value = max_label_value; this->ignore_strand = ignore_strand; this->preprocess = preprocess;
  if (win_step <= 0 || win_size % win_step != 0) { std::cerr << "Error: window size must be a multiple of window step in 'GenomicRegionSetScanner'!\n"; exit(1); }
  n_win_combine = win_size / win_step;
  cur_block = 0; cur_win = 0; computed = false; total_label_value = 0;
  halt_set = false; halt_block = 0; halt_win = 0; halt_line = 0; halt_no_prefix = false;
  keep_slot = g_keep_next; g_keep_next = -1;
}

GenomicRegionSetScanner::~GenomicRegionSetScanner() {}

void GenomicRegionSetScanner::Compute(bool sorted_rules)
{
  computed = true;
  if (win_step > INT_MAX || win_size > INT_MAX) { std::cerr << "Error: window geometry does not fit the MI355X path!\n"; exit(1); }
  ChromTable chroms;
  for (StringLIntMap::iterator p = bounds->begin(); p != bounds->end(); p++) chroms.Add(p->first.c_str());
  chroms.Freeze();
  const int n_chrom = chroms.size(), ns = ignore_strand ? 1 : 2;
  // iteration order of the reference: chromosomes in map order, '+' block then '-' block
  std::vector<int32_t> class_len((size_t)std::max(1, n_chrom * ns));
  std::vector<int64_t> class_off((size_t)std::max(1, n_chrom * ns));
  long long total = 0;
  chrom_names.clear(); n_windows.clear(); block_offset.clear();
  for (int r = 0; r < n_chrom; r++) {
    long int len = (*bounds)[chroms.name(r)];
    if (len >= INT_MAX - 1) { std::cerr << "Error: chromosome length does not fit the MI355X path!\n"; exit(1); }
    chrom_names.push_back(chroms.name(r));
    for (int s = 0; s < ns; s++) {
      long long nw = gtx_scan_n_windows(len < 0 ? 0 : len, win_step, win_size);
      class_len[(size_t)(s * n_chrom + r)] = (int32_t)(len < 0 ? 0 : len);
      class_off[(size_t)(s * n_chrom + r)] = total;
      n_windows.push_back((long int)nw); block_offset.push_back(total);
      total += nw;
    }
  }
  values.assign((size_t)std::max<long long>(keep_slot >= 0 ? 1 : total, 1), 0);
  if (n_chrom == 0) return;
  if (sorted_rules && preprocess == 'p') { ComputeMappable(class_len, class_off); return; }

  PackOptions opt;
  opt.mode = sorted_rules ? gtxhost::PACK_SCAN_SORTED : gtxhost::PACK_SCAN_UNSORTED;
  opt.chroms = &chroms; opt.strand_aware = !ignore_strand; opt.sorted_by_strand = !ignore_strand;
  opt.max_label_value = max_label_value;
  opt.keep_prefix_on_error = sorted_rules;
  PackError input_error;                                           // sorted rules: met where the reference's walk meets it (below), not here
  std::function<void(const PackError &)> on_error;
  if (sorted_rules) on_error = [&](const PackError &e) { input_error = e; };
  std::vector<int32_t> tri, w;
  bool bad_preprocess = false;                                     // raised at the first region that is processed, like the reference
  const bool preprocess_ok = sorted_rules ? preprocess == '1' : (preprocess == '1' || preprocess == 'c');
  const char prep = (preprocess == 'c' && !sorted_rules) ? 'c' : '1';
  const uint32_t rule_flags = sorted_rules ? GTX_ZERO_LENGTH_OK : 0u;
  gtx_group *grp = NULL;
  gtx_ctx *one = NULL;                                             // one GPU: the scan is fed as a stream (gtx_scan_begin .. gtx_scan_end)
  auto device_side = [&] {
    grp = Devices();
    if (gtx_group_size(grp) != 1) return;
    one = gtx_group_ctx(grp, 0);
    if (gtx_scan_begin(one, class_len.data(), n_chrom * ns, (int32_t)win_step, (int32_t)win_size, prep, rule_flags, max_label_value > 1, class_off.data()) != GTX_OK) {
      fflush(stdout); fprintf(stderr, "\nError: [gtx] %s\n", gtx_last_error(one)); exit(1);
    }
  };
  auto check_one = [&](int rc) { if (rc != GTX_OK) { fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, gtx_last_error(one)); exit(1); } };
  // the input's text tokenised on the device where that applies (one GPU, a streamed BED input: TextOnDevice)
  TextSink text_sink;
  text_sink.usable = [&] { return one != NULL; };
  text_sink.needs_host = [&](int ticket) { int redo = 0; check_one(gtx_text_result(one, ticket, &redo)); return redo != 0; };
  text_sink.add = [&](const char *text, size_t bytes, int64_t lines, const gtx_text_rules &rules, uint32_t text_flags) {
    if (!preprocess_ok) { bad_preprocess = true; g_drain_stop = true; return -1; }
    int ticket = -1;
    check_one(gtx_scan_add_text(one, text, bytes, lines, &rules, text_flags | ((sorted_rules || TextLooksSorted(text, bytes, text_flags & (GTX_TEXT_SAM | GTX_TEXT_GFF))) ? 0u : GTX_READS_UNSORTED), &ticket));
    return ticket;
  };
  DrainSet(R, opt, device_side, [&](const PackedBatch &b) {
    if (!preprocess_ok) { bad_preprocess = true; g_drain_stop = true; return; }
    total_label_value += (long int)b.label_sum;
    if (b.tri.empty()) return;
    if (one) { check_one(gtx_scan_add(one, b.tri.data(), b.w.empty() ? NULL : b.w.data(), (int64_t)(b.tri.size() / 3), LooksSorted(b.tri) ? 0u : GTX_READS_UNSORTED)); return; }
    tri.insert(tri.end(), b.tri.begin(), b.tri.end());
    w.insert(w.end(), b.w.begin(), b.w.end());
  }, &text_sink, on_error);
  if (input_error.set && !bad_preprocess) {
    // Where does the reference's walk fetch the offending line?  When it consumes the region in front of it (R->Next, :4944 / :4936):
    // inside that region's block at the micro-window its start falls into -- the windows whose last micro-window lies before that
    // one are out by then --, or, for a region no block takes (a chromosome without bounds, a start behind the last micro-window),
    // by the skip loop at the head of the first block behind it (:4934); a region behind every block is never consumed, and neither
    // is the line behind it met.  No region in front of the line: the constructor's first read meets it (:4882).
    const long int comb = win_size / win_step;
    halt_set = true; halt_block = 0; halt_win = 0;
    halt_line = input_error.line; halt_no_prefix = input_error.no_prefix; halt_msg = input_error.msg;
    if (input_error.have_last) {
      const size_t ci = (size_t)(std::lower_bound(chrom_names.begin(), chrom_names.end(), input_error.last_chrom) - chrom_names.begin());
      const bool known = ci < chrom_names.size() && chrom_names[ci] == input_error.last_chrom;
      size_t at_head_of = ci * (size_t)ns;                         // unknown chromosome: skipped at the head of the first block of a later one
      if (known) {
        const size_t B = ci * (size_t)ns + ((!ignore_strand && input_error.last_strand == '-') ? 1 : 0);
        const long int n_mw = std::max<long int>(0, (*bounds)[chrom_names[ci]]) / win_step;
        const long int k = input_error.last_start <= 0 ? 1 : (input_error.last_start + win_step - 1) / win_step;
        if (k <= n_mw) { halt_block = B; halt_win = std::max<long int>(0, std::min<long int>(k - comb, n_windows[B])); at_head_of = (size_t)-1; }
        else at_head_of = B + 1;
      }
      if (at_head_of != (size_t)-1) {
        if (at_head_of < n_windows.size()) { halt_block = at_head_of; halt_win = 0; }
        else halt_set = false;                                     // never consumed: the walk ends without meeting the line
      }
    }
  }
  if (bad_preprocess && sorted_rules) { fprintf(stderr, "Error: [SortedGenomicRegionSetScanner] preprocess operator '%c' not supported!\n", preprocess); exit(1); }
  if (bad_preprocess) { fprintf(stderr, "Error: [UnsortedGenomicRegionSetScanner] preprocess operator '%c' not supported!\n", preprocess); exit(1); }
  if (!grp) device_side();                                         // (an in-memory input: DrainSet has not run the hand-over's first step)
  if (one) {
    int64_t text_labels = 0;                                       // the lines the device took: their label values are summed there
    if (keep_slot >= 0) check_one(gtx_scan_end_keep(one, keep_slot, &text_labels));
    else check_one(gtx_scan_end(one, (uint64_t *)values.data(), &text_labels));
    total_label_value += (long int)text_labels;
    return;
  }
  if (keep_slot >= 0) { keep_error = "windows are kept on the device on one GPU only!"; return; }
  CheckGrp(grp, gtx_group_scan(grp, tri.data(), w.empty() ? NULL : w.data(), (int64_t)(tri.size() / 3), class_len.data(), n_chrom * ns,
                               (int32_t)win_step, (int32_t)win_size, prep, rule_flags | (LooksSortedVec(tri) ? GTX_READS_SORTED : 0u),
                               (uint64_t *)values.data(), class_off.data()));
}

// The sorted scanner's operator 'p' (genomic_intervals.cpp:4939-4942; what `genomic_scans peaks` scans its mappability track with): a
// micro-window receives the part of a region that lies at or below its stop -- and the walk behind it is what the reference wrote, not
// what one would expect: after a region that ends inside the micro-window it moves on twice (:4940, then :4945: the region behind it
// is never looked at), after one that reaches beyond the micro-window once, with the region's start set to stop + 1 by then (:4941):
// the rest of that region is dropped and the order check of the pull (:3879) sees the moved start.  Which region is looked at
// depends on every region before it, so this is a host-side walk over the set's own iterators (a mappability track is a secondary
// input, read once); what it yields is (block, micro-window, amount), and those go to the device as weighted point reads: the
// micro-window histogram and the window sums are the scan kernels' as for any other input.  An input error is met where the walk
// meets it (halt_*), like the sorted scanner's other errors.  One case the reference leaves undefined: the first of the two pulls
// meeting the end of the stream (its second pull deletes the last region again); the walk ends there here.
void GenomicRegionSetScanner::ComputeMappable(const std::vector<int32_t> &class_len, const std::vector<int64_t> &class_off)
{
  const int n_chrom = (int)chrom_names.size(), ns = ignore_strand ? 1 : 2;
  const bool by_strand = !ignore_strand;
  std::vector<int32_t> tri, w;
  auto emit = [&](int cls, long int mw, long int amount) {
    const int32_t pos = (int32_t)((mw - 1) * win_step + 1);          // a position of that micro-window
    while (amount != 0) {                                              // (a weight is 32 bits; an amount beyond that goes in pieces)
      const long int piece = std::max<long int>(INT_MIN + 1, std::min<long int>(INT_MAX, amount));
      tri.push_back(cls); tri.push_back(pos); tri.push_back(pos); w.push_back((int32_t)piece);
      amount -= piece;
    }
  };
  LoadError err;
  size_t at_block = 0; long int at_mw = 0;                             // where the walk is: what the halt position is read off
  tls_load_error = &err;
  try {
    GenomicRegion *r = R->Get();
    for (int c = 0; c < n_chrom && r; c++)
      for (int s = 0; s < ns && r; s++) {
        const char *chrom = chrom_names[(size_t)c].c_str();
        const char strand = s ? '-' : '+';
        at_block = (size_t)(c * ns + s); at_mw = 0;
        for (;;) {                                                     // the regions that sort before this block (:4934)
          if (!r) break;
          const int t = strcmp(chrom, r->I.front()->CHROMOSOME);
          if (!(t > 0 || (t == 0 && strand > r->I.front()->STRAND))) break;
          r = R->Next(by_strand, false);
        }
        const long int n_mw = (long int)class_len[(size_t)(s * n_chrom + c)] / win_step;
        while (r && strcmp(r->I.front()->CHROMOSOME, chrom) == 0 && (ignore_strand || r->I.front()->STRAND == strand)) {
          GenomicInterval *i = r->I.front();
          const long int first = i->START <= 0 ? 1 : (i->START + win_step - 1) / win_step;   // the first micro-window whose stop reaches the start
          if (std::max(first, at_mw) > n_mw) break;                    // (left for the skip loop of the next block)
          at_mw = std::max<long int>(std::max(first, at_mw), 1);
          if (r->I.size() != 1) r->PrintError("single-interval regions expected for this operation!\n");
          const long int stop = at_mw * win_step;
          if (i->STOP <= stop) {
            emit(s * n_chrom + c, at_mw, i->STOP - i->START + 1);
            r = R->Next(by_strand, false);
            if (!r) break;
          } else {
            emit(s * n_chrom + c, at_mw, stop - i->START + 1);
            i->START = stop + 1;
          }
          r = R->Next(by_strand, false);
        }
      }
  } catch (const LoadAbort &) {}
  tls_load_error = NULL;
  if (err.set) {
    const long int comb = win_size / win_step;
    halt_set = true; halt_line = err.line; halt_msg = err.msg; halt_no_prefix = !err.with_prefix;
    halt_block = at_block; halt_win = std::max<long int>(0, std::min<long int>(at_mw - comb, n_windows[at_block]));
  }
  gtx_group *grp = Devices();
  const int64_t n = (int64_t)w.size();
  const uint32_t order = LooksSortedVec(tri) ? 0u : GTX_READS_UNSORTED;
  if (gtx_group_size(grp) == 1) {
    gtx_ctx *one = gtx_group_ctx(grp, 0);
    auto check = [&](int rc) { if (rc != GTX_OK) { fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, gtx_last_error(one)); exit(1); } };
    check(gtx_scan_begin(one, class_len.data(), n_chrom * ns, (int32_t)win_step, (int32_t)win_size, '1', GTX_ZERO_LENGTH_OK, 1, class_off.data()));
    if (n) check(gtx_scan_add(one, tri.data(), w.data(), n, order));
    if (keep_slot >= 0) check(gtx_scan_end_keep(one, keep_slot, NULL));
    else check(gtx_scan_end(one, (uint64_t *)values.data(), NULL));
    return;
  }
  if (keep_slot >= 0) { keep_error = "windows are kept on the device on one GPU only!"; return; }
  CheckGrp(grp, gtx_group_scan(grp, tri.data(), w.data(), n, class_len.data(), n_chrom * ns, (int32_t)win_step, (int32_t)win_size, '1',
                               GTX_ZERO_LENGTH_OK | (order ? 0u : GTX_READS_SORTED), (uint64_t *)values.data(), class_off.data()));
}

void GenomicRegionSetScanner::KeepNextOnDevice(int slot)
{
  if (slot < 0 || slot >= GTX_SCAN_KEEP_SLOTS) { std::cerr << "Error: [GenomicRegionSetScanner] no such device slot!\n"; exit(1); }
  g_keep_next = slot;
}

void GenomicRegionSetScanner::BringKeptToHost()
{
  if (!computed) Compute(false);
  if (keep_slot < 0) return;
  if (!keep_error.empty()) { std::cerr << "Error: " << keep_error << "\n"; exit(1); }
  const long long total = WindowCount();
  if (total > 0) {
    gtx_ctx *one = gtx_group_ctx(Devices(), 0);
    values.assign((size_t)total, 0);
    if (gtx_scan_kept_read(one, keep_slot, (uint64_t *)values.data()) != GTX_OK || gtx_scan_drop(one, keep_slot) != GTX_OK) {   // (the slot's HBM is free again)
      fflush(stdout); fprintf(stderr, "\nError: [gtx] %s\n", gtx_last_error(one)); exit(1);
    }
  }
  keep_slot = -1;
}

long long GenomicRegionSetScanner::WindowCount()
{
  if (!computed) Compute(false);
  return block_offset.empty() ? 0 : block_offset.back() + n_windows.back();
}

void GenomicRegionSetScanner::PrintIntervalAt(FILE *out_file, long long window)
{
  if (!computed) Compute(false);
  const int ns = ignore_strand ? 1 : 2;
  const size_t b = (size_t)(std::upper_bound(block_offset.begin(), block_offset.end(), window) - block_offset.begin()) - 1;   // (empty blocks share an offset: the last one at or below holds it)
  const long long k = window - block_offset[b];
  fprintf(out_file, "%s %c %lld %lld", chrom_names[b / ns].c_str(), (b % ns) ? '-' : '+', (long long)win_step * k + 1, (long long)win_step * k + win_size);
}

bool GtxSelectWindows(GenomicRegionSetScanner **scanners, int n_tested, int n_control, const std::vector<std::vector<int> > &tables, long int win_size,
                      std::vector<long long> &ordinals, std::vector<int> &rows, std::string *error)
{
  ordinals.clear(); rows.clear();
  if (n_tested < 1 || n_tested > 4 || (n_control != 0 && n_control != n_tested) || (int)tables.size() != n_tested || win_size < 1 || win_size >= INT_MAX) {
    *error = "[GtxSelectWindows] one to four tested inputs, a control for each or for none, a table for each!"; return false;
  }
  gtx_group *grp = Devices();
  if (gtx_group_size(grp) != 1) { *error = "this operation runs on one GPU only!"; return false; }
  gtx_ctx *one = gtx_group_ctx(grp, 0);
  const void *d_vec[8] = {};
  const int32_t *tab[4] = {};
  long long n = -1;
  for (int f = 0; f < n_tested + n_control; f++) {
    const long long nf = scanners[f]->WindowCount();
    if (!scanners[f]->KeepError().empty()) { *error = scanners[f]->KeepError(); return false; }
    void *d = NULL; int64_t kept = 0;                                // (bounds without a window: nothing was scanned, nothing is selected)
    if (nf > 0 && (scanners[f]->KeptSlot() < 0 || gtx_scan_kept(one, scanners[f]->KeptSlot(), &d, &kept) != GTX_OK || (long long)kept != nf)) {
      *error = "[GtxSelectWindows] an input's windows are not on the device!"; return false;
    }
    if (n >= 0 && nf != n) { *error = "[GtxSelectWindows] the inputs differ in their number of windows!"; return false; }
    n = nf; d_vec[f] = d;
  }
  for (int f = 0; f < n_tested; f++) {
    if (tables[(size_t)f].size() != (size_t)(n_control ? win_size + 1 : 1)) { *error = "[GtxSelectWindows] a table of the wrong size!"; return false; }
    tab[f] = tables[(size_t)f].data();
  }
  const size_t cols = (size_t)(n_tested + n_control);
  int64_t cap = std::max<int64_t>(1 << 16, n / 64), kept = 0;        // a retry with the reported count when this was too small
  for (;;) {
    ordinals.resize((size_t)cap); rows.resize((size_t)cap * cols);
    const int rc = gtx_window_select(one, d_vec, n_control ? d_vec + n_tested : NULL, n_tested, n, (int32_t)win_size, tab, cap, (int64_t *)ordinals.data(), rows.data(), &kept);
    if (rc != GTX_OK) { *error = std::string("[gtx] ") + gtx_last_error(one); return false; }
    if (kept <= cap) break;
    cap = kept;
  }
  ordinals.resize((size_t)kept); rows.resize((size_t)kept * cols);
  return true;
}

bool GtxSelectPeakWindows(GenomicRegionSetScanner *signal, GenomicRegionSetScanner *control, GenomicRegionSetScanner *uniq, long int win_size, long int min_reads,
                          bool norm, double p_ratio, std::vector<long long> &ordinals, std::vector<long long> &rows, std::string *error)
{
  ordinals.clear(); rows.clear();
  if (signal == NULL || control == NULL || win_size < 1) { *error = "[GtxSelectPeakWindows] a signal, a control and a positive window size!"; return false; }
  gtx_group *grp = Devices();
  if (gtx_group_size(grp) != 1) { *error = "this operation runs on one GPU only!"; return false; }
  gtx_ctx *one = gtx_group_ctx(grp, 0);
  GenomicRegionSetScanner *scanners[3] = {signal, control, uniq};
  const void *d_vec[3] = {};
  long long n = -1;
  for (int f = 0; f < 3; f++) {
    if (scanners[f] == NULL) continue;
    const long long nf = scanners[f]->WindowCount();
    if (!scanners[f]->KeepError().empty()) { *error = scanners[f]->KeepError(); return false; }
    void *d = NULL; int64_t kept = 0;                                // (bounds without a window: nothing was scanned, nothing is selected)
    if (nf > 0 && (scanners[f]->KeptSlot() < 0 || gtx_scan_kept(one, scanners[f]->KeptSlot(), &d, &kept) != GTX_OK || (long long)kept != nf)) {
      *error = "[GtxSelectPeakWindows] an input's windows are not on the device!"; return false;
    }
    if (n >= 0 && nf != n) { *error = "[GtxSelectPeakWindows] the inputs differ in their number of windows!"; return false; }
    n = nf; d_vec[f] = d;
  }
  if (n == 0) return true;
  int64_t cap = std::max<int64_t>(1 << 16, n / 64), kept = 0;        // a retry with the reported count when this was too small
  for (;;) {
    ordinals.resize((size_t)cap); rows.resize((size_t)cap * 3);
    const int rc = gtx_peak_select(one, d_vec[0], d_vec[1], d_vec[2], n, win_size, min_reads, norm ? 1 : 0, p_ratio, cap, (int64_t *)ordinals.data(),
                                   (int64_t *)rows.data(), &kept);
    if (rc != GTX_OK) { *error = std::string("[gtx] ") + gtx_last_error(one); return false; }
    if (kept <= cap) break;
    cap = kept;
  }
  ordinals.resize((size_t)kept); rows.resize((size_t)kept * 3);
  return true;
}

long int GenomicRegionSetScanner::TotalLabelValue()
{
  if (!computed) Compute(false);
  return total_label_value;
}

// genomic_intervals.cpp:6206-6214: every region of the file, by the unsorted reader's rules (no order check; a line it cannot read
// ends the run), its label value capped.  The scanners deliver this sum with their windows (TotalLabelValue); this pass is for the
// caller that needs it although a sorted scanner stopped at an input error.
long int CountGenomicRegions(char *reg_file, long int max_label_value)
{
  GenomicRegionSet set(reg_file, 10000, false, false, true);
  ChromTable none; none.Freeze();
  PackOptions opt;
  opt.mode = gtxhost::PACK_SCAN_UNSORTED; opt.chroms = &none; opt.max_label_value = max_label_value;
  long int n = 0;
  DrainSet(&set, opt, [] {}, [&](const PackedBatch &b) { n += (long int)b.label_sum; });
  return n;
}

// genomic_intervals.cpp:6032-6040: the sizes of the regions' intervals, summed over the file by the plain reader
unsigned long int CalcRegSize(char *reg_file)
{
  GenomicRegionSet set(reg_file, 100000, false, false, true);
  unsigned long int n = 0;
  for (GenomicRegion *r = set.Get(); r != NULL; r = set.Next()) n += (unsigned long int)r->GetSize(true);
  return n;
}

unsigned long int CalcBoundSize(StringLIntMap *bounds)
{
  unsigned long int y = 0;
  for (StringLIntMap::iterator x = bounds->begin(); x != bounds->end(); x++) y += (unsigned long int)x->second;
  return y;
}

void GenomicRegionSetScanner::RaiseHalt()
{
  PackError e; e.set = true; e.line = halt_line; e.no_prefix = halt_no_prefix; e.msg = halt_msg;
  fflush(stdout);
  DiePack(e);
}

long int GenomicRegionSetScanner::Next()
{
  if (!computed) Compute(false);
  if (keep_slot >= 0) { std::cerr << "Error: [GenomicRegionSetScanner] the windows were kept on the device!\n"; exit(1); }
  while (cur_block < n_windows.size()) {
    if (halt_set && (cur_block > halt_block || (cur_block == halt_block && cur_win >= halt_win))) RaiseHalt();
    if (cur_win < n_windows[cur_block]) { cur_win++; return (long int)values[(size_t)(block_offset[cur_block] + cur_win - 1)]; }
    cur_block++; cur_win = 0;
  }
  if (halt_set) RaiseHalt();
  return -1;
}

void GenomicRegionSetScanner::PrintRemaining(FILE *out_file, long int min_value)
{
  if (!computed) Compute(false);
  if (keep_slot >= 0) { std::cerr << "Error: [GenomicRegionSetScanner] the windows were kept on the device!\n"; exit(1); }
  const int ns = ignore_strand ? 1 : 2;
  std::vector<char> buf; buf.reserve(8u << 20);
  auto put_num = [&](long int v) {
    char tmp[24]; int n = 0;
    unsigned long int u = v < 0 ? 0ul - (unsigned long int)v : (unsigned long int)v;
    do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) buf.push_back('-');
    while (n) buf.push_back(tmp[--n]);
  };
  for (; cur_block < n_windows.size(); cur_block++, cur_win = 0) {
    const std::string &chrom = chrom_names[cur_block / ns];
    const char strand = (cur_block % ns) ? '-' : '+';
    for (; cur_win < n_windows[cur_block]; cur_win++) {
      if (halt_set && (cur_block > halt_block || (cur_block == halt_block && cur_win >= halt_win))) goto done;
      const long int v = (long int)values[(size_t)(block_offset[cur_block] + cur_win)];
      if (v == -1) { cur_win++; goto done; }                      // (a caller's loop takes Next() == -1 for the end, whatever made the value)
      if (v < min_value) continue;
      put_num(v); buf.push_back('\t');
      buf.insert(buf.end(), chrom.begin(), chrom.end()); buf.push_back(' '); buf.push_back(strand); buf.push_back(' ');
      put_num(win_step * cur_win + 1); buf.push_back(' '); put_num(win_step * cur_win + win_size); buf.push_back('\n');
      if (buf.size() > (7u << 20)) { fwrite(buf.data(), 1, buf.size(), out_file); buf.clear(); }
    }
  }
done:
  if (!buf.empty()) fwrite(buf.data(), 1, buf.size(), out_file);
  if (halt_set && (cur_block >= n_windows.size() || cur_block > halt_block || (cur_block == halt_block && cur_win >= halt_win))) { fflush(out_file); RaiseHalt(); }
}

void GenomicRegionSetScanner::PrintFiltered(FILE *out_file, GenomicRegionSetIndex *index, long int min_value)
{
  if (!computed) Compute(false);
  if (keep_slot < 0) { std::cerr << "Error: [GenomicRegionSetScanner] the windows were not kept on the device!\n"; exit(1); }
  if (!keep_error.empty()) { std::cerr << "Error: " << keep_error << "\n"; exit(1); }
  const int n_chrom = (int)chrom_names.size(), ns = ignore_strand ? 1 : 2;
  const long long total = WindowCount();
  // a sorted scanner's input error: the windows in front of where the walk meets it, then the error
  const long long limit = halt_set ? std::min<long long>(total, block_offset[halt_block] + halt_win) : total;
  const unsigned long long floor_value = min_value < 0 ? 0ull : (unsigned long long)min_value;
  bool ended = false;                                              // at a value of -1 (PrintRemaining: a caller's loop takes it for the end)
  if (total > 0 && limit > 0) {
    gtx_ctx *one = gtx_group_ctx(Devices(), 0);
    auto check = [&](int rc) { if (rc != GTX_OK) { fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, gtx_last_error(one)); exit(1); } };
    void *d_windows = NULL; int64_t n_kept_windows = 0;
    check(gtx_scan_kept(one, keep_slot, &d_windows, &n_kept_windows));
    // the scan's classes (Compute: strand-major) over the blocks' offsets, and the index's regions in that numbering
    std::vector<int32_t> class_len((size_t)(n_chrom * ns));
    std::vector<int64_t> class_off((size_t)(n_chrom * ns));
    for (int r = 0; r < n_chrom; r++)
      for (int s = 0; s < ns; s++) {
        class_len[(size_t)(s * n_chrom + r)] = (int32_t)std::max<long int>(0, (*bounds)[chrom_names[(size_t)r]]);
        class_off[(size_t)(s * n_chrom + r)] = block_offset[(size_t)(r * ns + s)];
      }
    std::vector<int32_t> tri;
    GenomicRegionSet *set = index->regSet;
    for (long k = 0; k < set->n_regions; k++) {
      GenomicInterval *i = set->R[k]->I.front();
      if (i->STOP <= 0 || i->START > i->STOP || i->START >= INT_MAX) continue;   // never found (:5659), or behind every window
      const size_t ci = (size_t)(std::lower_bound(chrom_names.begin(), chrom_names.end(), std::string(i->CHROMOSOME)) - chrom_names.begin());
      if (ci >= chrom_names.size() || chrom_names[ci] != i->CHROMOSOME) continue;
      tri.push_back((int32_t)(((!ignore_strand && i->STRAND == '-') ? n_chrom : 0) + (int)ci));
      tri.push_back((int32_t)std::max<long int>(i->START, 1)); tri.push_back((int32_t)std::min<long int>(i->STOP, INT_MAX - 1));
    }
    check(gtx_window_refs(one, tri.data(), (int64_t)(tri.size() / 3), class_len.data(), class_off.data(), n_chrom * ns, (int32_t)win_step, (int32_t)win_size));
    std::vector<long long> ordinals;
    std::vector<unsigned long long> kept_values;
    int64_t cap = std::max<int64_t>(1 << 16, total / 64), kept = 0;    // a retry with the reported count when this was too small
    for (;;) {
      ordinals.resize((size_t)cap); kept_values.resize((size_t)cap);
      check(gtx_window_filter(one, d_windows, (int64_t)total, floor_value, cap, (int64_t *)ordinals.data(), (uint64_t *)kept_values.data(), &kept));
      if (kept <= cap) break;
      cap = kept;
    }
    std::vector<char> buf; buf.reserve(8u << 20);
    auto put_num = [&](long long v) {
      char tmp[24]; int n = 0;
      unsigned long long u = (unsigned long long)v;
      do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
      while (n) buf.push_back(tmp[--n]);
    };
    size_t b = 0;
    for (int64_t j = 0; j < kept; j++) {
      const long long at = ordinals[(size_t)j];
      if (at >= limit) break;
      const unsigned long long v = kept_values[(size_t)j];
      if (v == ~0ull) { ended = true; break; }
      if ((long long)v < 0) continue;                                // (a caller's loop compares as long int)
      while (b + 1 < block_offset.size() && block_offset[b + 1] <= at) b++;   // (empty blocks share an offset: the last one at or below holds it)
      const long long k = at - block_offset[b];
      const std::string &chrom = chrom_names[b / (size_t)ns];
      put_num((long long)v); buf.push_back('\t');
      buf.insert(buf.end(), chrom.begin(), chrom.end()); buf.push_back(' '); buf.push_back((b % (size_t)ns) ? '-' : '+'); buf.push_back(' ');
      put_num(win_step * k + 1); buf.push_back(' '); put_num(win_step * k + win_size); buf.push_back('\n');
      if (buf.size() > (7u << 20)) { fwrite(buf.data(), 1, buf.size(), out_file); buf.clear(); }
    }
    if (!buf.empty()) fwrite(buf.data(), 1, buf.size(), out_file);
  }
  cur_block = n_windows.size(); cur_win = 0;
  if (halt_set && !ended) { fflush(out_file); RaiseHalt(); }
}

void GenomicRegionSetScanner::PrintInterval(FILE *out_file)
{
  const int ns = ignore_strand ? 1 : 2;
  fprintf(out_file, "%s %c %ld %ld", chrom_names[cur_block / ns].c_str(), (cur_block % ns) ? '-' : '+', win_step * (cur_win - 1) + 1,
          win_step * (cur_win - 1) + win_size);
}

GenomicInterval *GenomicRegionSetScanner::GetInterval()
{
  const int ns = ignore_strand ? 1 : 2;
  return new GenomicInterval(chrom_names[cur_block / ns].c_str(), (cur_block % ns) ? '-' : '+', win_step * (cur_win - 1) + 1,
                             win_step * (cur_win - 1) + win_size);
}

// reference filter of `genomic_scans counts -r` through the reference's own iteration: windows are produced by the GPU scan as
// always; which of them are reported is a host-side question per window (at most one rank query or one merge step each).
// PrintFiltered answers the indexed form for all windows at once on the device.
long int GenomicRegionSetScanner::Next(GenomicRegionSet *Ref)
{
  if (Ref == NULL) return Next();
  GenomicRegion *q = Ref->Get();
  const bool sorted_by_strand = !ignore_strand;
  while (q != NULL) {
    const long int c = Next();
    if (c == -1) return -1;
    const int ns = ignore_strand ? 1 : 2;
    GenomicInterval w(chrom_names[cur_block / ns].c_str(), (cur_block % ns) ? '-' : '+', win_step * (cur_win - 1) + 1, win_step * (cur_win - 1) + win_size);
    while (q != NULL) {
      const int d = q->I.front()->CalcDirection(&w, sorted_by_strand);
      if (d < 0) q = Ref->Next(sorted_by_strand, false);
      else if (d == 0) return c;
      else break;
    }
  }
  return -1;
}

long int GenomicRegionSetScanner::Next(GenomicRegionSetIndex *index)
{
  if (index == NULL) return Next();
  while (true) {
    const long int c = Next();
    if (c == -1) return -1;
    const int ns = ignore_strand ? 1 : 2;
    GenomicInterval w(chrom_names[cur_block / ns].c_str(), (cur_block % ns) ? '-' : '+', win_step * (cur_win - 1) + 1, win_step * (cur_win - 1) + win_size);
    if (index->GetOverlap(&w, false, ignore_strand) != NULL) return c;
  }
}

// ---- GenomicRegionSetIndex ---------------------------------------------------------------------------
struct GenomicRegionSetIndex::Impl {
  struct Track { std::vector<long> start; std::vector<long> max_stop; std::vector<long> arg; };   // sorted by start; running max of stop
  std::map<std::string, Track> by_chrom[3];                       // 0: '+', 1: '-', 2: both strands
};

GenomicRegionSetIndex::GenomicRegionSetIndex(GenomicRegionSet *regSet, const char *)
{
  this->regSet = regSet;
  impl = new Impl;
  if (!regSet->load_in_memory) regSet->PrintError("[GenomicRegionSetIndex] the region set must be loaded in memory!");
  struct Item { long start, stop, k; };
  std::map<std::string, std::vector<Item>> items[3];
  for (long k = 0; k < regSet->n_regions; k++) {
    GenomicRegion *r = regSet->R[k];
    if (r->I.size() != 1) r->PrintError("multi-interval regions are outside the MI355X path!");
    GenomicInterval *i = r->I.front();
    if (i->STOP <= 0 || i->START > i->STOP) continue;              // never found (genomic_intervals.cpp:5659)
    items[i->STRAND == '-' ? 1 : 0][i->CHROMOSOME].push_back({i->START, i->STOP, k});
    items[2][i->CHROMOSOME].push_back({i->START, i->STOP, k});
  }
  for (int s = 0; s < 3; s++)
    for (auto &kv : items[s]) {
      std::stable_sort(kv.second.begin(), kv.second.end(), [](const Item &a, const Item &b) { return a.start < b.start; });
      Impl::Track &t = impl->by_chrom[s][kv.first];
      long best = LONG_MIN, who = -1;
      for (const Item &it : kv.second) {
        if (it.stop > best) { best = it.stop; who = it.k; }
        t.start.push_back(it.start); t.max_stop.push_back(best); t.arg.push_back(who);
      }
    }
}

GenomicRegionSetIndex::~GenomicRegionSetIndex() { delete impl; }

GenomicRegion *GenomicRegionSetIndex::GetOverlap(GenomicInterval *i, bool, bool ignore_strand)
{
  const auto &m = impl->by_chrom[ignore_strand ? 2 : (i->STRAND == '-' ? 1 : 0)];
  auto it = m.find(i->CHROMOSOME);
  if (it == m.end()) return NULL;
  const Impl::Track &t = it->second;
  // regions with start <= i->STOP; among them the largest stop must reach i->START
  const size_t n = (size_t)(std::upper_bound(t.start.begin(), t.start.end(), i->STOP) - t.start.begin());
  if (n == 0 || t.max_stop[n - 1] < i->START) return NULL;
  return regSet->R[t.arg[n - 1]];
}

SortedGenomicRegionSetScanner::SortedGenomicRegionSetScanner(GenomicRegionSet *R, StringLIntMap *bounds, long int win_step, long int win_size,
                                                             long int max_label_value, bool ignore_strand, char preprocess)
    : GenomicRegionSetScanner(R, bounds, win_step, win_size, max_label_value, ignore_strand, preprocess)
{
  Compute(true);
}

UnsortedGenomicRegionSetScanner::UnsortedGenomicRegionSetScanner(GenomicRegionSet *R, StringLIntMap *bounds, long int win_step, long int win_size,
                                                                 long int max_label_value, bool ignore_strand, char preprocess)
    : GenomicRegionSetScanner(R, bounds, win_step, win_size, max_label_value, ignore_strand, preprocess)
{
  Compute(false);
}

// the reference's scanners override the five virtuals (genomic_intervals.h:2291-2295, :2349-2353); here both run the shared body
#define GTX_SCANNER_OVERRIDES(CLS)                                                                                  \
  CLS::~CLS() {}                                                                                                    \
  void CLS::PrintInterval(FILE *out_file) { GenomicRegionSetScanner::PrintInterval(out_file); }                     \
  GenomicInterval *CLS::GetInterval() { return GenomicRegionSetScanner::GetInterval(); }                            \
  long int CLS::Next() { return GenomicRegionSetScanner::Next(); }                                                  \
  long int CLS::Next(GenomicRegionSet *Ref) { return GenomicRegionSetScanner::Next(Ref); }                          \
  long int CLS::Next(GenomicRegionSetIndex *index) { return GenomicRegionSetScanner::Next(index); }
GTX_SCANNER_OVERRIDES(SortedGenomicRegionSetScanner)
GTX_SCANNER_OVERRIDES(UnsortedGenomicRegionSetScanner)
#undef GTX_SCANNER_OVERRIDES

// ---------------------------------------------------------------------------------------------------
StringLIntMap *ReadBounds(char *genome_reg_file, bool verbose)
{
  if (genome_reg_file == NULL || strlen(genome_reg_file) == 0) { std::cerr << "Error: genome region file is necessary for this operation!\n"; exit(1); }
  StringLIntMap *bounds = new StringLIntMap();
  const bool gff_was = GtxAcceptGFF(false);                       // (a genome file is what it was: GFF is read as reads and reference regions only)
  GenomicRegionSet RegSet(genome_reg_file, 10000, verbose, false, true);
  GtxAcceptGFF(gff_was);
  long int line = 1;
  for (GenomicRegion *r = RegSet.Get(); r != NULL; r = RegSet.Next(), line++) {
    std::string chr = r->I.front()->CHROMOSOME;
    if (bounds->find(chr) == bounds->end()) (*bounds)[chr] = r->I.front()->STOP;
    else if ((*bounds)[chr] != r->I.front()->STOP) {
      std::cerr << "Error: chromosome " << chr << " has multiple lengths in genome file '" << genome_reg_file << "' line " << line << "!\n";
      exit(1);
    }
  }
  return bounds;
}

// ---------------------------------------------------------------------------------------------------
// genomic_overlaps overlap / intersect: the device join under the reference's per-query loop
// ---------------------------------------------------------------------------------------------------
namespace {
// what GenomicRegionBED::Print (genomic_intervals.cpp:2188-2220) needs of a query, kept until its batch is joined
struct PairQuery {
  std::string chrom, label, rgb;
  char strand;
  long int n_tokens, score, thick_start, thick_end;
  std::vector<long int> iv;                                        // start, stop of every interval
};

// columns 5, 7, 8, 9 of the raw line as GenomicRegionBED::Read takes them (:2157-2182: blank- or tab-separated, atol)
void ParseTail(const std::string &raw, PairQuery &q)
{
  const char sep = raw.find('\t') == std::string::npos ? ' ' : '\t';
  std::vector<std::string> tok;
  size_t k = 0;
  while (k < raw.size() && tok.size() < 9) {
    while (k < raw.size() && raw[k] == ' ') k++;
    size_t e = raw.find(sep, k);
    if (e == std::string::npos) e = raw.size();
    tok.push_back(raw.substr(k, e - k));
    k = e + 1;
  }
  q.score = tok.size() > 4 ? atol(tok[4].c_str()) : 0;
  q.thick_start = tok.size() > 7 ? atol(tok[6].c_str()) : 0;
  q.thick_end = tok.size() > 7 ? atol(tok[7].c_str()) : 0;
  q.rgb = tok.size() > 8 ? tok[8] : std::string();
}

void AppendNum(std::string &out, long int v) { char b[24]; int n = snprintf(b, sizeof b, "%ld", v); out.append(b, (size_t)n); }

// GenomicRegionBED::Print of a region with these intervals and this label
void PrintBed(std::string &out, const PairQuery &q, const std::vector<long int> &iv, const std::string &label, long int score,
              long int thick_start, long int thick_end)
{
  out += q.chrom; out += '\t'; AppendNum(out, iv[0] - 1); out += '\t'; AppendNum(out, iv.back());
  const long int nt = q.n_tokens;
  if (nt >= 4) {
    out += '\t'; out += label;
    if (nt >= 5) {
      out += '\t'; AppendNum(out, score);
      if (nt >= 6) {
        out += '\t'; out += q.strand;
        if (nt >= 8) {
          out += '\t'; AppendNum(out, thick_start); out += '\t'; AppendNum(out, thick_end);
          if (nt >= 9) {
            out += '\t'; out += q.rgb;
            if (nt == 12) {
              const size_t n = iv.size() / 2;
              out += '\t'; AppendNum(out, (long int)n); out += '\t';
              for (size_t j = 0; j < n; j++) { AppendNum(out, iv[2 * j + 1] - iv[2 * j] + 1); if (j + 1 < n) out += ','; }
              out += "\t0";
              for (size_t j = 1; j < n; j++) { out += ','; AppendNum(out, iv[2 * j] - iv[0]); }
            }
          }
        }
      }
    }
  }
  out += '\n';
}

bool FitsPacked(long int v) { return v < INT_MAX - 1 && v > INT_MIN + 1; }

// the index side of the join: classes (chromosome rank in strcmp order, x2 + strand unless -i), envelopes, intervals, order keys
struct JoinIndex {
  GenomicRegionSet *IS;
  bool sorted, ignore_strand;
  long int M;
  std::map<std::string, int> cid;
  int n_classes;
  std::vector<int32_t> tri, blocks; std::vector<int64_t> first;
  bool multi = false;                                                   // some region has more than one interval
  std::set<std::string> valid_chrom;                                    // chromosomes the bin index has (a valid region on them)
  std::vector<GenomicRegion *> regs;                                    // the regions by ordinal: the index set's, then (annotate) the upstream set's
  long int n_primary = 0;                                               // ordinals below it are the index set's
  gtx_ctx *ctx = NULL;
  bool strand_major = false;                                            // classes as the device-side tokenizer numbers them: rank, + chromosomes on '-' (set before BuildJoinIndex)
  int ClassOf(const GenomicInterval *i) const
  {
    std::map<std::string, int>::const_iterator it = cid.find(i->CHROMOSOME);
    if (it == cid.end()) return -1;
    if (ignore_strand) return it->second;
    return strand_major ? it->second + (i->STRAND == '-' ? (int)cid.size() : 0) : it->second * 2 + (i->STRAND == '-');
  }
  void Chk(int rc) const { if (rc != GTX_OK) { fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, gtx_last_error(ctx)); exit(1); } }
};

const size_t kQueryBatch = 1 << 20;                                     // queries per device call of the drivers

// the queries RunQueryLoop hands out, as gtx_join takes them, and the strand of each one's front interval
struct QueryBatch {
  std::vector<int32_t> qtri, qblk; std::vector<int64_t> qfirst = {0}; std::vector<int8_t> qstrand;
  bool qmulti = false;                                                  // some query has more than one interval
  void Add(const JoinIndex &ix, GenomicRegion *q)
  {
    GenomicInterval *f = q->I.front();
    for (GenomicInterval *i : q->I) { qblk.push_back((int32_t)i->START); qblk.push_back((int32_t)i->STOP); }
    if (q->I.size() > 1) qmulti = true;
    qfirst.push_back((int64_t)qblk.size() / 2);
    qtri.push_back(ix.ClassOf(f)); qtri.push_back((int32_t)f->START); qtri.push_back((int32_t)q->I.back()->STOP);
    qstrand.push_back(f->STRAND == '-' ? '-' : '+');
  }
  void Clear() { qtri.clear(); qblk.clear(); qfirst.assign(1, 0); qstrand.clear(); qmulti = false; }
  int64_t Size() const { return (int64_t)qstrand.size(); }
  const int64_t *First() const { return qmulti ? qfirst.data() : NULL; }
};

// gtx_join of the batch into off / pairs; when the pairs did not fit, pairs grows to them and the join runs again
void JoinPairs(const JoinIndex &ix, const QueryBatch &qb, uint32_t flags, std::vector<int64_t> &off, std::vector<int32_t> &pairs)
{
  const int64_t n = qb.Size();
  off.assign((size_t)n + 1, 0);
  if (pairs.empty()) pairs.resize(1 << 16);
  gtx_count_info info;
  auto join = [&]() { ix.Chk(gtx_join(ix.ctx, qb.qtri.data(), qb.First(), qb.qblk.data(), n, flags, off.data(), pairs.data(), (int64_t)pairs.size(), &info)); };
  join();
  if (off[n] > (int64_t)pairs.size()) { pairs.resize((size_t)off[n]); join(); }
}

// gtx_join_offsets of the batch into off / pairs / eoff / ent; returns the first inverted pair.  When the pairs did not fit, pairs
// and eoff grow (and ent, one entry per pair, unless skipping gaps) and the call runs again; then the same for the entries.
int64_t JoinOffsets(const JoinIndex &ix, const QueryBatch &qb, const int8_t *strands, uint32_t flags, int32_t op, std::vector<int64_t> &off,
                    std::vector<int32_t> &pairs, std::vector<int64_t> &eoff, std::vector<int64_t> &ent)
{
  const int64_t n = qb.Size();
  off.assign((size_t)n + 1, 0);
  if (pairs.empty()) { pairs.resize(1 << 16); eoff.resize(pairs.size() + 1); ent.resize(2 * pairs.size()); }
  int64_t inverted = -1;
  auto join = [&]() {
    ix.Chk(gtx_join_offsets(ix.ctx, qb.qtri.data(), qb.First(), qb.qblk.data(), strands, n, flags, op, off.data(), pairs.data(), (int64_t)pairs.size(),
                            eoff.data(), ent.data(), (int64_t)ent.size() / 2, &inverted, NULL));
  };
  join();
  const int64_t np = off[n];
  if (np > (int64_t)pairs.size()) {
    pairs.resize((size_t)np); eoff.resize((size_t)np + 1);
    if (!(flags & GTX_OFFSET_SKIP_REF_GAPS)) ent.resize(2 * (size_t)np);
    join();
  }
  if (eoff[np] > (int64_t)ent.size() / 2) { ent.resize(2 * (size_t)eoff[np]); join(); }
  return inverted;
}

// gtx_set_ref_strands: the strand of each index region's front interval
void SetRefStrands(const JoinIndex &ix)
{
  std::vector<int8_t> strand((size_t)std::max<long int>(ix.M, 1), '+');
  for (long int k = 0; k < ix.M; k++) strand[k] = ix.regs[k]->I.front()->STRAND == '-' ? '-' : '+';
  ix.Chk(gtx_set_ref_strands(ix.ctx, strand.data()));
}

// the text so far to stdout once it is longer than `above`
void WriteOut(std::string &out, size_t above = 0)
{
  if (out.size() > above) { fwrite(out.data(), 1, out.size(), stdout); out.clear(); }
}

// the index set of the overlaps object on the device (gtx_set_refs_ex, gtx_set_ref_order; the caller sets the blocks).  With
// single_if_invalid a region that is not compatible, sorted and non-overlapping is given its envelope alone: no pair of it can be
// printed (the bin index raises its error at the first query, the merge treats it as below), and its intervals may not be what
// gtx_set_ref_blocks accepts.
//
// `second` (annotate's upstream set, NULL otherwise) follows the index set as ordinals n_primary ..: one reference set on the device,
// in which the bin index's order key is the rank of (set, level, bin, -ordinal within its own set) -- each set's own iteration
// order (every region of the index set first), so one join returns a query's pairs as the reference's two walks hand them out.
void BuildJoinIndex(GenomicRegionSetOverlaps *ov, bool ignore_strand, const char *bin_bits, bool single_if_invalid, JoinIndex &ix,
                    GenomicRegionSet *second = NULL)
{
  // the per-pair operations print query lines as BED text (and read their BED columns back): a SAM set of the class API's is refused
  // here, with the message the CLIs give for it (GtxAcceptSAM); so is a GFF set
  for (GenomicRegionSet *s : {ov->QuerySet, ov->IndexSet})
    if (s->format == "SAM" || s->format == "GFF") ov->QuerySet->PrintError("unsupported input format!\n");
  GenomicRegionSet *IS = ov->IndexSet;
  ix.n_primary = IS->n_regions;
  ix.regs.assign(IS->R, IS->R + IS->n_regions);
  if (second) ix.regs.insert(ix.regs.end(), second->R, second->R + second->n_regions);
  const std::vector<GenomicRegion *> &R = ix.regs;
  const long int M = (long int)R.size();
  ix.IS = IS; ix.M = M; ix.ignore_strand = ignore_strand;
  ix.sorted = dynamic_cast<SortedGenomicRegionSetOverlaps *>(ov) != NULL;
  for (long int k = 0; k < M; k++) ix.cid[R[k]->I.front()->CHROMOSOME] = 0;
  { int n = 0; for (auto &c : ix.cid) c.second = n++; }
  ix.n_classes = std::max<int>(1, (int)ix.cid.size() * (ignore_strand ? 1 : 2));
  // under the merge an index region out of order or with overlapping blocks is the reference's error when the merge pulls it
  // (LoadIndexBuffer): the regions from there on can pair with no query before that error, so they are placeholders here
  long int v = M;
  if (ix.sorted) {
    const bool by_strand = static_cast<SortedGenomicRegionSetOverlaps *>(ov)->sorted_by_strand;
    for (long int k = 0; k < M && v == M; k++)
      if (!R[k]->IsCompatibleSortedAndNonoverlapping() || (k > 0 && R[k]->IsBefore(R[k - 1], by_strand))) v = k;
  }
  ix.tri.assign((size_t)3 * std::max<long int>(M, 1), 0); ix.first.assign((size_t)M + 1, 0);
  for (long int k = 0; k < M; k++) {
    GenomicRegion *r = R[k];
    const long int s = r->I.front()->START, e = r->I.back()->STOP;
    if (k >= v) { ix.tri[3 * k] = -1; ix.tri[3 * k + 1] = 1; ix.tri[3 * k + 2] = 0; ix.blocks.push_back(1); ix.blocks.push_back(0); ix.first[k + 1] = (int64_t)ix.blocks.size() / 2; continue; }
    if (!FitsPacked(s) || !FitsPacked(e)) r->PrintError("coordinate does not fit the packed 32-bit representation of the MI355X path!");
    ix.tri[3 * k] = ix.ClassOf(r->I.front()); ix.tri[3 * k + 1] = (int32_t)s; ix.tri[3 * k + 2] = (int32_t)e;
    if (single_if_invalid && r->I.size() > 1 && !r->IsCompatibleSortedAndNonoverlapping()) { ix.blocks.push_back((int32_t)s); ix.blocks.push_back((int32_t)e); }
    else {
      if (r->I.size() > 1) ix.multi = true;
      for (GenomicInterval *i : r->I) { ix.blocks.push_back((int32_t)i->START); ix.blocks.push_back((int32_t)i->STOP); }
    }
    ix.first[k + 1] = (int64_t)ix.blocks.size() / 2;
    if (!(s > e || e <= 0)) ix.valid_chrom.insert(r->I.front()->CHROMOSOME);
  }
  std::vector<int64_t> key;
  if (!ix.sorted) {                                                   // the bin index's order: (level, bin, -ordinal) (:5619-5674, :5729-5764)
    std::vector<int> bits;
    std::string bb = bin_bits ? bin_bits : "";
    if (bb.empty()) bits = {17, 20, 23, 26, 60};
    else {
      size_t p = 0;
      for (;;) { size_t q = bb.find(',', p); bits.push_back(atoi(bb.substr(p, q == std::string::npos ? q : q - p).c_str())); if (q == std::string::npos) break; p = q + 1; }
      bits.push_back(60);
    }
    struct LB { long int set, level, bin, k; };
    std::vector<LB> lb((size_t)M);
    for (long int k = 0; k < M; k++) {
      long int s = R[k]->I.front()->START; const long int e = R[k]->I.back()->STOP;
      if (s <= 0) s = 1;
      lb[k] = {k >= ix.n_primary, (long int)bits.size(), 0, k};
      for (size_t l = 0; l < bits.size(); l++) if ((s >> bits[l]) == (e >> bits[l])) { lb[k] = {k >= ix.n_primary, (long int)l, s >> bits[l], k}; break; }
    }
    std::sort(lb.begin(), lb.end(), [](const LB &a, const LB &b) {
      return a.set != b.set ? a.set < b.set : (a.level != b.level ? a.level < b.level : (a.bin != b.bin ? a.bin < b.bin : a.k > b.k));
    });
    key.resize((size_t)std::max<long int>(M, 1));
    for (long int j = 0; j < M; j++) key[lb[j].k] = j;
  }
  ix.ctx = gtx_group_ctx(Devices(), 0);
  ix.Chk(gtx_set_refs_ex(ix.ctx, ix.tri.data(), M, ix.n_classes, ix.sorted ? GTX_REFS_KEEP_ZERO_LENGTH : 0));
  ix.Chk(gtx_set_ref_order(ix.ctx, ix.sorted ? NULL : key.data()));
}

// What the caller's operation does with the merge per query, and when its loop ends.  overlap, intersect, offset and the signal
// bins walk every match and stop at Done(); subset (gtools/genomic_overlaps.cpp:794-795) calls GetOverlap once -- which erases from
// the merge's buffer only what lies in front of the first accepted match (:5903-5918), and Done() looks at that buffer (:5934-5937)
// -- and with -inv goes on while there is a query.
// annotate has no overlaps object: its loop reads the test set itself (gtools/genomic_overlaps.cpp:332) and asks a
// GenomicRegionSetIndex, whose constructor has checked the index regions before the loop and which answers a query with
// stop <= 0 or start > stop with no match instead of an error (:5500-5501) -- `index_rules`.
struct LoopWalk { bool single = false, match_gaps = false, ignore_strand = false, past_done = false, index_rules = false; };

// the reference's query loop on the overlaps object: errors, the merge's buffer and Done() (its early stop) come from the class
// layer, on which the caller's walk is replayed; add(q) takes every query in order.  Returns with err set when the loop stopped at
// an error.
void RunQueryLoop(GenomicRegionSetOverlaps *ov, const JoinIndex &ix, LoadError &err, const std::function<void(GenomicRegion *)> &add,
                  const LoopWalk &walk = LoopWalk())
{
  tls_load_error = &err;
  try {
    bool index_checked = ix.sorted || walk.index_rules;
    for (GenomicRegion *q = walk.index_rules ? ov->QuerySet->Get() : ov->GetQuery(); walk.index_rules || walk.past_done ? q != NULL : ov->Done() == false;
         q = walk.index_rules ? ov->QuerySet->Next() : ov->NextQuery()) {
      if (!index_checked) {                                               // the bin index is built at the first query's match (:5603-5616)
        for (long int k = 0; k < ix.M; k++)
          if (!ix.regs[k]->IsCompatibleSortedAndNonoverlapping()) ix.regs[k]->PrintError("index regions should be compatible, sorted and non-overlapping!");
        index_checked = true;
      }
      GenomicInterval *f = q->I.front();
      const long int s = f->START, e = q->I.back()->STOP;
      if (ix.sorted) {                                                    // the merge's buffer as the reference's walk leaves it
        if (walk.single) ov->GetOverlap(walk.match_gaps, walk.ignore_strand);
        else for (GenomicRegion *r = ov->GetMatch(); r; r = ov->NextMatch()) {}
      }
      else if (!walk.index_rules && ix.valid_chrom.count(f->CHROMOSOME)) { // :5740-5741, on chromosomes the index knows
        if (e <= 0) q->PrintError("stop position must be positive!");
        if (s > e) q->PrintError("start position cannot be greater than stop position!");
      }
      if (!FitsPacked(s) || !FitsPacked(e)) q->PrintError("coordinate does not fit the packed 32-bit representation of the MI355X path!");
      add(q);
    }
  } catch (const LoadAbort &) {}
  tls_load_error = NULL;
}

// the error the loop stopped at, as the reference prints it (after the output before it)
void ExitOnLoadError(const LoadError &err)
{
  fflush(stdout);
  if (!err.set) return;
  fprintf(stderr, "\n");
  if (err.with_prefix) fprintf(stderr, "Error: Line %ld: %s\n", err.line, err.msg.c_str()); else fprintf(stderr, "%s\n", err.msg.c_str());
  exit(1);
}
}  // namespace

void GtxPrintPairs(GenomicRegionSetOverlaps *ov, bool intersect, bool match_gaps, bool ignore_strand, bool merge_labels, const char *bin_bits)
{
  GenomicRegionSet *IS = ov->IndexSet, *QS = ov->QuerySet;
  if (!IS->load_in_memory) { fprintf(stderr, "Error: [GtxPrintPairs] the index set must be loaded in memory!\n"); exit(1); }
  if (QS->format == "GTX") { fprintf(stderr, "Error: overlap / intersect print the query lines: a packed region file has no labels, give the BED text!\n"); exit(1); }
  JoinIndex ix;
  BuildJoinIndex(ov, ignore_strand, bin_bits, false, ix);
  gtx_ctx *ctx = ix.ctx;
  ix.Chk(gtx_set_ref_blocks(ctx, ix.multi && !match_gaps ? ix.first.data() : NULL, ix.blocks.data()));
  const uint32_t flags = (ix.sorted ? GTX_ZERO_LENGTH_OK : 0) | (match_gaps ? GTX_JOIN_GAPS : 0);

  // ---- query side: batches of the queries the loop hands out, joined and printed in order ----
  std::vector<PairQuery> batch; batch.reserve(4096);
  QueryBatch qb;
  std::vector<int64_t> off; std::vector<int32_t> pairs;
  std::string out;
  auto flush = [&]() {
    const int64_t n = qb.Size();
    if (n == 0) return;
    JoinPairs(ix, qb, flags, off, pairs);
    std::vector<long int> civ;
    for (int64_t i = 0; i < n; i++) {
      const PairQuery &q = batch[i];
      for (int64_t p = off[i]; p < off[i + 1]; p++) {
        GenomicRegion *r = IS->R[pairs[p]];
        const std::string label = merge_labels ? q.label + ":" + r->LABEL : q.label;
        if (!intersect) PrintBed(out, q, q.iv, label, q.score, q.thick_start, q.thick_end);
        else {                                                              // Constrain (:2543-2561), match_gaps = false
          const long int rs = r->I.front()->START, re = r->I.back()->STOP;
          civ.clear();
          for (size_t j = 0; j < q.iv.size(); j += 2) {
            const long int a = std::max(q.iv[j], rs), b = std::min(q.iv[j + 1], re);
            if (a <= b) { civ.push_back(a); civ.push_back(b); }
          }
          if (civ.empty()) continue;
          PrintBed(out, q, civ, label, q.n_tokens >= 5 ? q.score : 0, q.n_tokens >= 7 ? std::max(q.thick_start, rs - 1) : rs - 1,
                   q.n_tokens >= 8 ? std::min(q.thick_end, re) : re);
        }
        WriteOut(out, 1u << 22);
      }
    }
    WriteOut(out);
    batch.clear(); qb.Clear();
  };

  LoadError err;
  RunQueryLoop(ov, ix, err, [&](GenomicRegion *q) {
    GenomicInterval *f = q->I.front();
    PairQuery pq;
    pq.chrom = f->CHROMOSOME; pq.strand = f->STRAND; pq.label = q->LABEL;
    pq.n_tokens = static_cast<GenomicRegionBED *>(q)->n_tokens;
    ParseTail(QS->CurrentLine(), pq);
    for (GenomicInterval *i : q->I) { pq.iv.push_back(i->START); pq.iv.push_back(i->STOP); }
    qb.Add(ix, q);
    batch.push_back(std::move(pq));
    if (batch.size() >= kQueryBatch) flush();
  });
  flush();                                                                // the pairs before an error are printed, then the error
  ExitOnLoadError(err);
}

// ---------------------------------------------------------------------------------------------------
// genomic_subset: hits per query from the device (gtx_query_hits), or the file's text selected there (gtx_subset_text)
// ---------------------------------------------------------------------------------------------------
namespace {
// May the test set's text go to the device as it is?  A streamed, uncompressed BED file (32 MB or more, or GTX_TEXT_ON_DEVICE=1;
// never with GTX_TEXT_ON_DEVICE=0) on one GPU, over an index set in which the loop could find no error of its own: every region
// compatible, sorted and non-overlapping, and under the merge the set in order.
bool SubsetTextUsable(GenomicRegionSetOverlaps *ov, const JoinIndex &ix, bool by_strand)
{
  static const char *e = getenv("GTX_TEXT_ON_DEVICE");
  GenomicRegionSet *QS = ov->QuerySet;
  if ((e && atoi(e) == 0) || QS->load_in_memory || QS->format != "BED" || QS->file == NULL || QS->from_stdin) return false;
  const long left = QS->StreamBytesLeft();
  if (left < ((e && atoi(e) == 1) ? 1 : (32l << 20))) return false;                    // (-1: stdin, .gz)
  if (gtx_group_size(Devices()) != 1) return false;
  if (g_pool_future.valid()) g_pool_future.get();
  if (!g_pool.buf[0] || !g_pool.buf[1]) return false;
  for (long int k = 0; k < ix.M; k++) {
    if (!ix.IS->R[k]->IsCompatibleSortedAndNonoverlapping()) return false;
    if (ix.sorted && k > 0 && ix.IS->R[k]->IsBefore(ix.IS->R[k - 1], by_strand)) return false;
  }
  return true;
}

// The test set's file block by block through gtx_subset_text, the selected text to stdout in block order.  Returns 0 when the
// whole file went that way, else the file line of the first block that came back: what the loop has to do from there on.
long int SubsetText(GenomicRegionSet *QS, const JoinIndex &ix, bool by_strand, uint32_t flags)
{
  gtx_ctx *ctx = ix.ctx;
  std::string first; long int first_no = 0;
  LineSource *src = QS->DetachStream(&first, &first_no);
  if (first_no <= 0) return 0;                                             // no region in the file
  ChromTable chroms;
  for (const auto &c : ix.cid) chroms.Add(c.first.c_str());
  chroms.Freeze();
  std::vector<const char *> names((size_t)chroms.size());
  for (int i = 0; i < chroms.size(); i++) names[i] = chroms.name(i).c_str();
  PackOptions opt;
  opt.mode = ix.sorted ? gtxhost::PACK_OVERLAPS_SORTED : gtxhost::PACK_OVERLAPS_UNSORTED;
  opt.chroms = &chroms; opt.strand_aware = !ix.ignore_strand; opt.sorted_by_strand = by_strand;
  gtx_text_rules rules;
  rules.chrom_names = names.empty() ? NULL : names.data(); rules.n_chrom = chroms.size();
  rules.strand_aware = opt.strand_aware; rules.sorted_rules = ix.sorted; rules.sorted_by_strand = by_strand; rules.max_label_value = 1;
  BedPacker packer(src, opt);
  // the line the set's constructor has read for its format check: packed here for what it says to the block behind it (the seam's
  // key; an error of its own is the loop's to report), and a block of one line for the device
  long int takeover = 0, takeover_block = 0, on_device = 0, n_blocks = 0, block_no[2] = {1, 1};
  auto report = [&]() {
    if (!getenv("GTX_TEXT_TRACE")) return;
    if (takeover) fprintf(stderr, "[gtx subset] blocks selected on the device: %ld, the loop took over at block %ld (line %ld)\n", on_device, takeover_block, takeover);
    else fprintf(stderr, "[gtx subset] blocks selected on the device: %ld, none came back\n", on_device);
  };
  packer.Prime(first, first_no);
  {
    PackedBatch batch; PackError err;
    packer.PackPrimedText(&batch, &err);
    if (err.set) { takeover = first_no; takeover_block = 1; report(); return takeover; }
  }
  g_pool.used[0] = g_pool.used[1] = true;                                  // (the buffers hold text now)
  packer.UseTextBuffers((char *)g_pool.buf[0], (char *)g_pool.buf[1], kPoolBytes);
  first += '\n';
  BedPacker::TextBlock blk[2]; int ticket[2] = {-1, -1};
  char *out = NULL; size_t out_cap = 0;
  auto settle = [&](int k) {                                               // the verdict on the block in blk[k]; what it selected goes out
    if (ticket[k] < 0) return;
    if (blk[k].bytes > out_cap) {
      if (out) gtx_host_free(ctx, out);
      out_cap = blk[k].bytes + (blk[k].bytes >> 3);
      out = (char *)gtx_host_alloc(ctx, out_cap);
      if (!out) ix.Chk(GTX_E_HIP);
    }
    int redo = 0; size_t got = 0;
    ix.Chk(gtx_subset_result(ctx, ticket[k], &redo, out, &got, NULL));
    ticket[k] = -1;
    if (takeover) return;                                                  // (a block behind the one that came back: the loop's)
    if (redo) { takeover = blk[k].first_line; takeover_block = block_no[k]; return; }
    if (blk[k].text != first.data()) on_device++;
    if (got) fwrite(out, 1, got, stdout);
  };
  auto add = [&](int k) {
    const BedPacker::TextBlock &b = blk[k];
    rules.have_prev = b.have_prev; rules.prev_chrom = b.prev_chrom.c_str(); rules.prev_strand = b.prev_strand; rules.prev_start = b.prev_start;
    ix.Chk(gtx_subset_text(ctx, b.text, b.bytes, b.n_lines, &rules, flags, &ticket[k]));
  };
  blk[0].text = &first[0]; blk[0].bytes = first.size(); blk[0].first_line = first_no; blk[0].n_lines = 1; blk[0].have_prev = false;
  add(0);
  int cur = 1;
  for (;; cur ^= 1) {
    settle(cur);                                                           // (its buffer is about to be read over)
    if (takeover) break;
    if (!packer.NextTextBlock(&blk[cur])) break;
    block_no[cur] = ++n_blocks;
    if (!blk[cur].seam_ok) {                                               // a block behind a last line that could not be read: no key for the order check at the seam
      settle(cur ^ 1);
      if (!takeover) { takeover = blk[cur].first_line; takeover_block = n_blocks; }
      break;
    }
    add(cur);
  }
  settle(cur); settle(cur ^ 1);                                            // (the older block first)
  if (out) gtx_host_free(ctx, out);
  g_pool.used[0] = g_pool.used[1] = false;
  report();
  return takeover;
}
}  // namespace

void GtxPrintSubset(GenomicRegionSetOverlaps *ov, bool match_gaps, bool ignore_strand, bool inverse, const char *bin_bits)
{
  GenomicRegionSet *IS = ov->IndexSet, *QS = ov->QuerySet;
  if (!IS->load_in_memory) { fprintf(stderr, "Error: [GtxPrintSubset] the index set must be loaded in memory!\n"); exit(1); }
  if (QS->format == "GTX") { fprintf(stderr, "Error: subset prints the query lines: a packed region file has no labels, give the BED text!\n"); exit(1); }
  JoinIndex ix;
  ix.strand_major = true;
  BuildJoinIndex(ov, ignore_strand, bin_bits, false, ix);
  gtx_ctx *ctx = ix.ctx;
  ix.Chk(gtx_set_ref_blocks(ctx, ix.multi && !match_gaps ? ix.first.data() : NULL, ix.blocks.data()));
  const uint32_t flags = (ix.sorted ? GTX_ZERO_LENGTH_OK : 0) | (match_gaps ? GTX_JOIN_GAPS : 0);
  const bool by_strand = ix.sorted && static_cast<SortedGenomicRegionSetOverlaps *>(ov)->sorted_by_strand;

  // ---- the text path: whole blocks selected on the device; the first one that comes back hands the rest of the file to the loop,
  // which reads the file again from its start -- silently up to that block, so that the merge's cursor, buffer and previous query
  // are what they would have been -- on a set and an overlaps object of its own
  long int resume = 0;                                                    // the loop prints the queries from this file line on
  GenomicRegionSet *again = NULL; GenomicRegionSetOverlaps *again_ov = NULL;
  if (SubsetTextUsable(ov, ix, by_strand)) {
    resume = SubsetText(QS, ix, by_strand, flags | (inverse ? GTX_SUBSET_INVERT : 0));
    if (resume == 0) { fflush(stdout); return; }
    again = new GenomicRegionSet(QS->file, QS->buffer_size, QS->verbose, false, true);
    if (ix.sorted) again_ov = new SortedGenomicRegionSetOverlaps(again, IS, by_strand);
    else again_ov = new UnsortedGenomicRegionSetOverlaps(again, IS, bin_bits);
    ov = again_ov; QS = again;
  }

  // ---- the loop: batches of the queries it hands out, their hits from the device, the selected ones printed in order ----
  std::vector<PairQuery> batch; batch.reserve(4096);
  QueryBatch qb;
  std::vector<uint32_t> hits;
  std::string out;
  auto flush = [&]() {
    const int64_t n = qb.Size();
    if (n == 0) return;
    hits.resize((size_t)n);
    ix.Chk(gtx_query_hits(ctx, qb.qtri.data(), qb.First(), qb.qblk.data(), n, flags, hits.data(), NULL));
    for (int64_t i = 0; i < n; i++) {
      if ((hits[i] == 0) != inverse) continue;
      const PairQuery &q = batch[i];
      PrintBed(out, q, q.iv, q.label, q.score, q.thick_start, q.thick_end);
      WriteOut(out, 1u << 22);
    }
    WriteOut(out);
    batch.clear(); qb.Clear();
  };

  LoopWalk walk;
  walk.single = true; walk.match_gaps = match_gaps; walk.ignore_strand = ignore_strand; walk.past_done = inverse;
  LoadError err;
  RunQueryLoop(ov, ix, err, [&](GenomicRegion *q) {
    if (q->n_line < resume) return;
    GenomicInterval *f = q->I.front();
    PairQuery pq;
    pq.chrom = f->CHROMOSOME; pq.strand = f->STRAND; pq.label = q->LABEL;
    pq.n_tokens = static_cast<GenomicRegionBED *>(q)->n_tokens;
    ParseTail(QS->CurrentLine(), pq);
    for (GenomicInterval *i : q->I) { pq.iv.push_back(i->START); pq.iv.push_back(i->STOP); }
    qb.Add(ix, q);
    batch.push_back(std::move(pq));
    if (batch.size() >= kQueryBatch) flush();
  }, walk);
  flush();                                                                // what was selected before an error is printed, then the error
  ExitOnLoadError(err);
  delete again_ov; delete again;
}

// ---------------------------------------------------------------------------------------------------
// genomic_overlaps offset: the device join and its pair offsets under the reference's per-query loop
// ---------------------------------------------------------------------------------------------------
namespace {
// printf("%ld %ld") / ("%f %f") / -c of one entry (gtools/genomic_overlaps.cpp:566-575): float division by a size_t size
void AppendOffsets(std::string &out, long int a, long int b, size_t size, bool fraction, bool center)
{
  char buf[160];
  int n;
  if (center) n = fraction ? snprintf(buf, sizeof buf, "%f", ((float)a / size + (float)b / size) / 2) : snprintf(buf, sizeof buf, "%ld", (a + b) / 2);
  else n = fraction ? snprintf(buf, sizeof buf, "%f %f", (float)a / size, (float)b / size) : snprintf(buf, sizeof buf, "%ld %ld", a, b);
  out.append(buf, (size_t)std::min<int>(n, (int)sizeof buf - 1));
}

// what a line needs of a query, kept until its batch is joined
struct OffsetQuery { std::string label; long int n_line; size_t n_intervals; long int start, stop; };
}  // namespace

void GtxPrintOffsets(GenomicRegionSetOverlaps *ov, const char *op, bool skip_ref_gaps, bool fraction, bool center, bool print_labels,
                     bool match_gaps, bool ignore_strand, const char *bin_bits)
{
  GenomicRegionSet *IS = ov->IndexSet;
  if (!IS->load_in_memory) { fprintf(stderr, "Error: [GtxPrintOffsets] the index set must be loaded in memory!\n"); exit(1); }
  JoinIndex ix;
  BuildJoinIndex(ov, ignore_strand, bin_bits, true, ix);
  gtx_ctx *ctx = ix.ctx;
  const bool sorted = ix.sorted;
  // the reference point's front / back intervals and strand: the index regions' unless -S, where the merge's queries are the
  // reference file (its branch :545-583) and the index regions' envelopes are offset
  ix.Chk(gtx_set_ref_blocks(ctx, ix.multi ? ix.first.data() : NULL, ix.blocks.data()));
  SetRefStrands(ix);
  const std::string ops = op;
  const int32_t code = ops == "1" ? GTX_OFFSET_1 : ops == "2" ? GTX_OFFSET_2 : ops == "5p" ? GTX_OFFSET_5P : ops == "3p" ? GTX_OFFSET_3P : 0;
  const uint32_t flags = (sorted ? GTX_ZERO_LENGTH_OK | GTX_OFFSET_FROM_QUERY : 0) | (match_gaps ? GTX_JOIN_GAPS : 0) |
                         (skip_ref_gaps ? GTX_OFFSET_SKIP_REF_GAPS : 0);
  // GetSize of the reference region: the envelope (:1047-1055), with --skip-ref-gaps the sum of its intervals (GetSize() of an
  // interval: 0 when inverted, :488-491)
  auto ref_size = [&](GenomicRegion *r) -> size_t {
    if (!skip_ref_gaps) return r->I.back()->STOP - r->I.front()->START + 1;
    size_t z = 0;
    for (GenomicInterval *i : r->I) z += i->START > i->STOP ? 0 : i->STOP - i->START + 1;
    return z;
  };
  std::vector<size_t> isize((size_t)std::max<long int>(ix.M, 1));
  for (long int k = 0; k < ix.M; k++) isize[k] = ref_size(IS->R[k]);

  std::vector<OffsetQuery> batch; batch.reserve(4096);
  QueryBatch qb;
  std::vector<int64_t> off, eoff, ent; std::vector<int32_t> pairs;
  std::string out;
  auto die = [&](const char *msg) { WriteOut(out); fflush(stdout); fprintf(stderr, "%s", msg); exit(1); };
  auto die_line = [&](long int n_line, const char *msg) {
    WriteOut(out); fflush(stdout); fprintf(stderr, "\nError: Line %ld: %s\n", n_line, msg); exit(1);
  };
  auto flush = [&]() {
    const int64_t n = qb.Size();
    if (n == 0) return;
    const int64_t inverted = JoinOffsets(ix, qb, sorted ? qb.qstrand.data() : NULL, flags, code ? code : GTX_OFFSET_1, off, pairs, eoff, ent);
    for (int64_t i = 0; i < n; i++) {
      const OffsetQuery &q = batch[i];
      for (int64_t p = off[i]; p < off[i + 1]; p++) {
        GenomicRegion *r = IS->R[pairs[p]];
        if (skip_ref_gaps) {                                                // :634-670: a line only for a pair with entries
          if (eoff[p + 1] == eoff[p]) continue;
          if (!code) die("Error: unknown offset reference point operation!\n");
          out += r->LABEL; out += '\t';
          if (print_labels) { out += q.label; out += ' '; }
          for (int64_t e = eoff[p]; e < eoff[p + 1]; e++) AppendOffsets(out, ent[2 * e], ent[2 * e + 1], isize[pairs[p]], fraction, center);
        } else {
          // :556-576 (-S: the query is the reference region, r the test region) and :604-624
          if (sorted ? r->I.size() > 1 : q.n_intervals > 1) die_line(sorted ? r->n_line : q.n_line, "multi-interval test regions are not allowed for this operation!");
          out += sorted ? q.label.c_str() : r->LABEL; out += '\t';
          if (print_labels) { out += sorted ? r->LABEL : q.label.c_str(); out += ' '; }
          if (!code) die("Error: unknown offset reference point operation!\n");
          if (p == inverted) die("Error: start offset is greater than stop offset (this must be a bug)!\n");
          const size_t size = sorted ? (size_t)(q.stop - q.start + 1) : isize[pairs[p]];
          AppendOffsets(out, ent[2 * eoff[p]], ent[2 * eoff[p] + 1], size, fraction, center);
        }
        out += '\n';
        WriteOut(out, 1u << 22);
      }
    }
    WriteOut(out);
    batch.clear(); qb.Clear();
  };

  LoadError err;
  RunQueryLoop(ov, ix, err, [&](GenomicRegion *q) {
    batch.push_back(OffsetQuery{q->LABEL, q->n_line, q->I.size(), q->I.front()->START, q->I.back()->STOP});
    qb.Add(ix, q);
    if (batch.size() >= kQueryBatch) flush();
  });
  flush();
  ExitOnLoadError(err);
}

// ---------------------------------------------------------------------------------------------------
// genomic_overlaps annotate: the upstream builder (host), and the device join with its annotate pass under the reference's loop
// ---------------------------------------------------------------------------------------------------
GenomicRegionSet *CreateGenomicRegionSetAnnotator(GenomicRegionSet *RefRegSet, StringLIntMap *bounds, bool ignore_strand, long int upstream_max_distance,
                                                  long int upstream_min_distance, char *bin_bits)
{
  auto make = [](const std::string &label, GenomicInterval *of, long int start, long int stop, long int n_line) {
    GenomicRegion *u = new GenomicRegion();
    u->n_line = n_line;
    u->LABEL = CopyString(label.c_str());
    u->I.push_back(new GenomicInterval(of->CHROMOSOME, of->STRAND, start, stop, n_line));
    return u;
  };
  const char *range_msg = "upstream region does not fit the packed 32-bit representation of the MI355X path!";
  // one upstream region per reference region (:6231-6241)
  std::vector<GenomicRegion *> up;
  std::vector<GenomicRegion *> gene;                                      // the region each one was made from (error lines)
  for (GenomicRegion *ireg = RefRegSet->Get(); ireg != NULL; ireg = RefRegSet->Next()) {
    if (ireg->I.size() != 1) ireg->PrintError("single-interval reference regions are required for this operation!");
    GenomicInterval *i = ireg->I[0];
    const bool plus = i->STRAND == '+';
    const long int new_start = plus ? std::max(i->START - upstream_max_distance, 1L) : i->STOP + 1;
    long int new_stop = plus ? std::max(i->START - 1, 1L) : i->STOP + upstream_max_distance;
    if (bounds) new_stop = std::min(new_stop, (*bounds)[i->CHROMOSOME]);  // (operator[]: an unnamed chromosome is inserted with 0)
    if (!FitsPacked(new_start) || !FitsPacked(new_stop)) ireg->PrintError(range_msg);
    up.push_back(make(std::string("upstream:") + ireg->LABEL, i, new_start, new_stop, (long int)up.size() + 1));
    gene.push_back(ireg);
  }
  RefRegSet->Reset();
  GenomicRegionSet *U = new GenomicRegionSet(up);
  if (!(upstream_min_distance < upstream_max_distance)) return U;

  // a non-overlapping set (:6250-6294): every region against the untrimmed set, through that set's bin index
  std::vector<GenomicRegion *> kept;
  {
    UnsortedGenomicRegionSetOverlaps self(U, U, bin_bits);
    long int k = 0;
    for (GenomicRegion *ureg = self.GetQuery(); ureg != NULL; ureg = self.NextQuery(), k++) {
      GenomicInterval *u = ureg->I[0];
      long int start = u->START, stop = u->STOP;
      const bool asks = !(stop <= 0 || start > stop);                     // GenomicRegionSetIndex::NextMatch (:5500-5501): no match, no error
      for (GenomicRegion *r = asks ? self.GetOverlap(true, ignore_strand) : NULL; r != NULL; r = self.NextOverlap(true, ignore_strand)) {
        GenomicInterval *o = r->I[0];
        if (o == u) continue;
        if (u->STRAND != o->STRAND) continue;
        if (u->STRAND == '+') {
          if (u->STOP > o->STOP) {
            start = std::max(start, o->STOP + 1);
            if (upstream_min_distance > 0 && stop - start + 1 < upstream_min_distance) start = std::max(1L, stop - upstream_min_distance + 1);
          }
        } else if (o->START > u->START) {
          stop = std::min(stop, o->START - 1);
          if (upstream_min_distance > 0 && stop - start + 1 < upstream_min_distance) {
            stop = start + upstream_min_distance - 1;
            if (bounds) stop = std::min(stop, (*bounds)[o->CHROMOSOME]);
          }
        }
        if (start > stop) break;
      }
      if (start <= stop) {
        if (!FitsPacked(start) || !FitsPacked(stop)) gene[(size_t)k]->PrintError(range_msg);
        kept.push_back(make(ureg->LABEL, u, start, stop, (long int)kept.size() + 1));
      }
    }
  }
  delete U;
  return new GenomicRegionSet(kept);
}

namespace {
// what a line needs of a test region, kept until its batch is joined
struct AnnotateQuery { std::string label, chrom; char strand; long int start, stop, n_line; };

// "%s %c %ld %ld" of PrintInterval and "%lu" of the interval's size
void AppendLocus(std::string &out, const char *chrom, char strand, long int start, long int stop)
{
  out += chrom; out += ' '; out += strand; out += ' '; AppendNum(out, start); out += ' '; AppendNum(out, stop);
  char b[32]; const int n = snprintf(b, sizeof b, "\t%lu\t", (unsigned long int)(stop - start + 1)); out.append(b, (size_t)n);
}

// PrintAnnotations (gtools/genomic_overlaps.cpp:277-289) of one printed pair; offset as the reference's double
void AppendAnnotation(std::string &out, const AnnotateQuery &q, GenomicRegion *ireg, bool three_prime, double offset, bool flag, long int proximal_dist)
{
  out += q.label; out += '\t';
  AppendLocus(out, q.chrom.c_str(), q.strand, q.start, q.stop);
  if (flag) {
    if (three_prime) { out += offset >= proximal_dist ? "distal" : "proximal"; out += ':'; }
    else { out += offset > proximal_dist ? "distal" : "proximal"; out += ":downstream:"; }
  }
  GenomicInterval *i = ireg->I[0];
  out += ireg->LABEL; out += '\t';
  AppendLocus(out, i->CHROMOSOME, i->STRAND, i->START, i->STOP);
  char b[400]; const int n = snprintf(b, sizeof b, "%ld\t%f\n", (long int)offset, offset / ireg->GetSize(false));
  out.append(b, (size_t)std::min<int>(n, (int)sizeof b - 1));
}

// GenomicInterval::GetOffsetFrom(GenomicRegion *) (:646-667) on the host, for the walk over plain pairs
void HostOffsetFrom(GenomicRegion *ref, bool three_prime, long int s, long int e, long int *so, long int *eo)
{
  const bool minus = ref->I.front()->STRAND == '-';
  const bool back = minus != three_prime;                                 // -5p and +3p: the back interval, its stop
  GenomicInterval *iv = back ? ref->I.back() : ref->I.front();
  const long int point = back ? iv->STOP : iv->START;
  if (back) { *so = point - e; *eo = point - s; } else { *so = s - point; *eo = e - point; }
}
}  // namespace

void GtxPrintAnnotations(GenomicRegionSet *TestRegSet, GenomicRegionSet *RefRegSet, GenomicRegionSet *UpstreamRefRegSet, const char *query_op,
                         bool ignore_strand, bool distance_flag, long int proximal_dist, bool print_header, const char *bin_bits)
{
  if (!RefRegSet->load_in_memory || (UpstreamRefRegSet && !UpstreamRefRegSet->load_in_memory)) {
    fprintf(stderr, "Error: [GtxPrintAnnotations] the reference sets must be loaded in memory!\n"); exit(1);
  }
  // the constructor of the reference's index (:5365), before anything is printed
  for (GenomicRegionSet *set : {RefRegSet, UpstreamRefRegSet})
    for (long int k = 0; set && k < set->n_regions; k++)
      if (!set->R[k]->IsCompatibleSortedAndNonoverlapping()) set->R[k]->PrintError("index regions should be compatible, sorted and non-overlapping!");
  UnsortedGenomicRegionSetOverlaps ov(TestRegSet, RefRegSet, bin_bits);
  JoinIndex ix;
  BuildJoinIndex(&ov, ignore_strand, bin_bits, true, ix, UpstreamRefRegSet);
  gtx_ctx *ctx = ix.ctx;
  ix.Chk(gtx_set_ref_blocks(ctx, NULL, NULL));                            // (match_gaps = true, :318: envelopes)
  SetRefStrands(ix);
  const std::string op = query_op;
  const bool center = op == "center", known = center || op == "overlap";
  bool multi_ref = false;                                                 // a pair may reach a multi-interval reference region: plain pairs, walked here
  for (GenomicRegion *r : ix.regs) if (r->I.size() != 1) multi_ref = true;
  const uint32_t flags = GTX_JOIN_GAPS;
  const int32_t mode = center ? GTX_ANNOTATE_CENTER : GTX_ANNOTATE_START;   // (an unknown word ends the run at the first pair: every pair is kept)

  if (print_header) { StdoutIsOurs(); printf("TEST-LABEL\tTEST-LOCUS\tTEST-LOCUS-SIZE\tREF-LABEL\tREF-LOCUS\tREF-LOCUS-SIZE\tOFFSET\tNORMALIZED-OFFSET\n"); }

  std::vector<AnnotateQuery> batch; batch.reserve(4096);
  QueryBatch qb;
  std::vector<int64_t> koff, kval, off; std::vector<int32_t> kref, pairs;
  std::string out;
  auto die = [&](const char *msg) { WriteOut(out); fflush(stdout); fprintf(stderr, "%s", msg); exit(1); };
  auto flush = [&]() {
    const int64_t n = qb.Size();
    if (n == 0) return;
    if (multi_ref) {
      JoinPairs(ix, qb, flags, off, pairs);
      for (int64_t i = 0; i < n; i++) {
        const AnnotateQuery &q = batch[i];
        for (int64_t p = off[i]; p < off[i + 1]; p++) {
          GenomicRegion *r = ix.regs[pairs[p]];
          if (r->I.size() != 1) { WriteOut(out); fflush(stdout); fprintf(stderr, "\nError: Line %ld: %s\n", r->n_line, "single-interval reference regions are required for this operation!"); exit(1); }
          const bool three_prime = pairs[p] >= ix.n_primary;
          long int so, eo;
          HostOffsetFrom(r, three_prime, q.start, q.stop, &so, &eo);
          double offset = 0;
          if (center) { offset = (double)(so + eo) / 2; if (offset < 0) continue; }
          else if (known) offset = (double)so;
          else die("Error [PrintAnnotations]: invalid value for query operation!\n");
          AppendAnnotation(out, q, r, three_prime, offset, distance_flag, proximal_dist);
          WriteOut(out, 1u << 22);
        }
      }
    } else {
      koff.assign((size_t)n + 1, 0);
      if (kref.empty()) { kref.resize(1 << 16); kval.resize(kref.size()); }
      auto join = [&]() {
        ix.Chk(gtx_join_annotate(ctx, qb.qtri.data(), n, flags, ix.n_primary, GTX_OFFSET_5P, GTX_OFFSET_3P, mode, koff.data(), kref.data(), kval.data(),
                                 (int64_t)kref.size(), NULL, NULL));
      };
      join();
      if (koff[n] > (int64_t)kref.size()) { kref.resize((size_t)koff[n]); kval.resize(kref.size()); join(); }
      for (int64_t i = 0; i < n; i++) {
        const AnnotateQuery &q = batch[i];
        for (int64_t p = koff[i]; p < koff[i + 1]; p++) {
          if (!known) die("Error [PrintAnnotations]: invalid value for query operation!\n");
          const double offset = center ? (double)kval[p] / 2 : (double)kval[p];
          AppendAnnotation(out, q, ix.regs[kref[p]], kref[p] >= ix.n_primary, offset, distance_flag, proximal_dist);
          WriteOut(out, 1u << 22);
        }
      }
    }
    WriteOut(out);
    batch.clear(); qb.Clear();
  };

  LoopWalk walk;
  walk.index_rules = true;
  LoadError err;
  RunQueryLoop(&ov, ix, err, [&](GenomicRegion *q) {
    if (q->I.size() != 1) q->PrintError("single-interval test regions are required for this operation!");
    GenomicInterval *f = q->I[0];
    batch.push_back(AnnotateQuery{q->LABEL, f->CHROMOSOME, f->STRAND, f->START, f->STOP, q->n_line});
    qb.Add(ix, q);
    if (f->STOP <= 0 || f->START > f->STOP) qb.qtri[qb.qtri.size() - 3] = -1;   // the index answers such a query with no match (:5500-5501)
    if (batch.size() >= kQueryBatch) flush();
  }, walk);
  flush();
  ExitOnLoadError(err);
}

// ---------------------------------------------------------------------------------------------------
// genomic_apps profile / heatmap: the signal bins under the reference's per-query loop
// ---------------------------------------------------------------------------------------------------
unsigned long int GtxSignalBins(GenomicRegionSetOverlaps *ov, const GtxSignalSpec &spec, std::vector<double> &bins)
{
  GenomicRegionSet *IS = ov->IndexSet;
  if (!IS->load_in_memory) { fprintf(stderr, "Error: [GtxSignalBins] the reference set must be loaded in memory!\n"); exit(1); }
  JoinIndex ix;
  BuildJoinIndex(ov, spec.ignore_strand, "17,20,23,26", true, ix);
  gtx_ctx *ctx = ix.ctx;
  const long int M = ix.M, B = spec.n_bins;
  ix.Chk(gtx_set_ref_blocks(ctx, ix.multi ? ix.first.data() : NULL, ix.blocks.data()));
  SetRefStrands(ix);
  // ref_len: GetSize(SKIP_REF_GAPS) under --norm-ref-length (a size_t), else 1
  std::vector<int64_t> ref_len((size_t)std::max<long int>(M, 1), 1);
  if (spec.norm_ref_len) for (long int k = 0; k < M; k++) ref_len[k] = (int64_t)IS->R[k]->GetSize(spec.skip_ref_gaps);
  ix.Chk(gtx_set_signal_bins(ctx, spec.bin_min, spec.bin_max, B, spec.norm_ref_len ? ref_len.data() : NULL));
  const uint32_t flags = spec.per_ref ? GTX_SIGNAL_PER_REF : 0;
  const size_t len = (size_t)std::max<long int>(0, (spec.per_ref ? M : 1) * B);

  // integral weights accumulate exactly in int64 on the device; from the first fractional weight on (and under --skip-ref-gaps
  // from the start) the host adds doubles in the reference's order, starting from the exact integer sums
  std::vector<int64_t> ibins(len, 0);
  bins.assign(len, 0.0);
  bool host = spec.skip_ref_gaps;
  int64_t abs_sum = 0;
  const char *kInverted = "Error: start offset is greater than stop offest (this must be a bug)!\n";
  auto add = [&](long int r, long int a, long int b, double w) {
    const double x = (double)(a + b) / 2 / (size_t)ref_len[r] + spec.bin_min;
    const double z = (double)(x - spec.bin_min) / (spec.bin_max - spec.bin_min);
    if ((z >= 0) && (z < 1)) {
      const int bin = (int)(B * z);
      if (bin < B) bins[(spec.per_ref ? (size_t)r * B : 0) + bin] += w;   // bin == n_bins: past the reference's array, dropped
    }
  };

  QueryBatch qb;
  std::vector<int64_t> qw, off, eoff, ent; std::vector<double> qwd;
  std::vector<int32_t> pairs;
  bool qfrac = false;
  unsigned long int n_signal_reg = 0;
  auto flush = [&]() {
    const int64_t n = qb.Size();
    if (n == 0) return;
    if (!host && qfrac) { host = true; for (size_t k = 0; k < len; k++) bins[k] = (double)ibins[k]; }
    if (!host) {
      int64_t inverted = -1; gtx_signal_info info;
      ix.Chk(gtx_signal_bins(ctx, qb.qtri.data(), qb.First(), qb.qblk.data(), spec.max_label_value <= 1 ? NULL : qw.data(), n, flags,
                             ibins.data(), &inverted, &info));
      if (inverted >= 0) { fflush(stdout); fprintf(stderr, "%s", kInverted); exit(1); }
      abs_sum += info.weight_abs_sum;
      if (abs_sum >= (int64_t)1 << 53) { fprintf(stderr, "Error: the label values summed into the bins reach 2^53: this build bins them exactly only below that!\n"); exit(1); }
    } else {
      // pairs only: the offsets of the front interval here; under --skip-ref-gaps CalcOffsetsWithoutGaps entries, in its loop order
      if (!spec.skip_ref_gaps) JoinPairs(ix, qb, 0, off, pairs);
      else JoinOffsets(ix, qb, NULL, GTX_OFFSET_SKIP_REF_GAPS, GTX_OFFSET_5P, off, pairs, eoff, ent);
      for (int64_t i = 0; i < n; i++) {
        const int32_t *fq = qb.qblk.data() + 2 * qb.qfirst[i];              // qreg->I.front()
        for (int64_t p = off[i]; p < off[i + 1]; p++) {
          const long int r = pairs[p];
          if (spec.skip_ref_gaps) { for (int64_t e = eoff[p]; e < eoff[p + 1]; e++) add(r, ent[2 * e], ent[2 * e + 1], qwd[i]); continue; }
          GenomicRegion *R = IS->R[r];
          const bool minus = R->I.front()->STRAND == '-';
          GenomicInterval *ri = minus ? R->I.back() : R->I.front();         // GetOffsetFrom(ireg, "5p")
          long int a, b;
          if (minus) { a = ri->STOP - fq[1]; b = ri->STOP - fq[0]; } else { a = fq[0] - ri->START; b = fq[1] - ri->START; }
          if (a > b) { fflush(stdout); fprintf(stderr, "%s", kInverted); exit(1); }
          add(r, a, b, qwd[i]);
        }
      }
    }
    qb.Clear(); qw.clear(); qwd.clear(); qfrac = false;
  };

  LoadError err;
  RunQueryLoop(ov, ix, err, [&](GenomicRegion *q) {
    n_signal_reg++;
    qb.Add(ix, q);
    // GetLabelValue(double) (:1072-1076)
    const double w = spec.max_label_value <= 1 ? 1 : std::min(spec.max_label_value, atof(q->LABEL));
    const bool integral = w == w && fabs(w) <= 2147483647.0 && w == (double)(int64_t)w;
    qwd.push_back(w); qw.push_back(integral ? (int64_t)w : 0);
    if (!integral) qfrac = true;
    if (qwd.size() >= kQueryBatch) flush();
  });
  flush();
  ExitOnLoadError(err);
  if (!host) for (size_t k = 0; k < len; k++) bins[k] = (double)ibins[k];
  return n_signal_reg;
}

// ---------------------------------------------------------------------------------------------------
// GenomicRegionSet::RunGlobalLink (genomic_intervals.cpp:4605-4644) on the device
// ---------------------------------------------------------------------------------------------------
namespace {

// the regions of a set, column by column, up to the first line the loop cannot take: `stop` says why it ends there.  want_score: the
// score column beside them (NULL for a line with fewer than 5 tokens).  front_of_multi: a multi-interval line that
// IsCompatibleSortedAndNonoverlapping (:1153-1161) is taken with its front interval -- what RunGlobalTest compares -- and one that is
// not ends the columns (UNSORTED_MULTI).
struct LinkColumns {
  bool want_score = false, front_of_multi = false;
  std::vector<const char *> chrom, label, score;
  std::vector<char> strand;
  std::vector<long> start, stop, line;
  enum Stop { NONE, MALFORMED, MULTI, UNSORTED_MULTI } why = NONE;
  long stop_line = 0; std::string stop_msg; bool stop_prefix = true;            // MALFORMED: the reader's message
  const char *stop_chrom = NULL; char stop_strand = '+'; long stop_start = 0;   // MULTI: the front interval (Next's order check comes first)
  std::vector<char> text;                                                        // what the pointers of a streamed set point into
  size_t size() const { return start.size(); }
  void append(const LinkColumns &o)
  {
    chrom.insert(chrom.end(), o.chrom.begin(), o.chrom.end()); label.insert(label.end(), o.label.begin(), o.label.end());
    strand.insert(strand.end(), o.strand.begin(), o.strand.end()); start.insert(start.end(), o.start.begin(), o.start.end());
    stop.insert(stop.end(), o.stop.begin(), o.stop.end()); line.insert(line.end(), o.line.begin(), o.line.end());
    score.insert(score.end(), o.score.begin(), o.score.end());
  }
};

// lines [b, e) of a block (every one ends in '\n'), numbered from `first`: parsed in place as GenomicRegionBED does
void LinkParsePiece(char *b, char *e, long first, LinkColumns *out)
{
  long no = first;
  for (char *q = b; q < e; no++) {
    char *nl = (char *)memchr(q, '\n', (size_t)(e - q));
    if (!nl) break;
    *nl = 0;
    gtxhost::BedFields f; char *bad = NULL;
    const gtxhost::BedStatus st = gtxhost::ParseBedLine(q, &f, &bad);
    q = nl + 1;
    if (st != gtxhost::BED_OK) {
      out->why = LinkColumns::MALFORMED; out->stop_line = no;
      if (st == gtxhost::BED_TOO_FEW_TOKENS) out->stop_msg = "number of tokens should be at least 3 for BED format!";
      else { out->stop_msg = std::string("Error: invalid strand '") + bad + "'!"; out->stop_prefix = false; }
      return;
    }
    long s = f.start, t = f.stop;
    if (f.n_tokens == 12) {
      std::vector<long> iv; gtxhost::BedBlocks(f, &iv);
      if (iv.size() < 2) { out->why = LinkColumns::MALFORMED; out->stop_line = no; out->stop_msg = "BED12 line without blocks!"; return; }
      if (iv.size() > 2 && !out->front_of_multi) { out->why = LinkColumns::MULTI; out->stop_line = no; out->stop_chrom = f.chrom; out->stop_strand = f.strand; out->stop_start = iv[0]; return; }
      for (size_t k = 2; k < iv.size(); k += 2)
        if (iv[k] < iv[k - 2] || iv[k] <= iv[k - 1]) { out->why = LinkColumns::UNSORTED_MULTI; out->stop_line = no; return; }
      s = iv[0]; t = iv[1];
    }
    if (s < -(long)INT_MAX || s > (long)INT_MAX || t < -(long)INT_MAX || t > (long)INT_MAX) {
      out->why = LinkColumns::MALFORMED; out->stop_line = no; out->stop_msg = "coordinate outside the 32-bit range of the MI355X path!"; return;
    }
    out->chrom.push_back(f.chrom); out->label.push_back(f.label ? f.label : "_"); out->strand.push_back(f.strand);
    out->start.push_back(s); out->stop.push_back(t); out->line.push_back(no);
    if (out->want_score) out->score.push_back(f.score);
  }
}

bool LinkBefore(const char *ca, char sa, long a, const char *cb, char sb, long b, bool by_strand)     // GenomicInterval::IsBefore (:396-401)
{
  const int c = strcmp(ca, cb);
  if (c != 0) return c < 0;
  if (by_strand && sa != sb) return sa < sb;
  return a < b;
}

// -?[1-9][0-9]* or 0: the labels whose atof() is the integer the device folds
bool LinkCanonicalInteger(const char *s, long long *v)
{
  const char *p = s;
  if (*p == '-') p++;
  if (*p < '0' || *p > '9' || (*p == '0' && (p[1] || p != s))) return false;
  const char *d = p;
  while (*p >= '0' && *p <= '9') p++;
  if (*p || p - d > 15) return false;                                            // (15 digits: below 2^53 whatever they are)
  *v = atoll(s);
  return true;
}

void LinkPutNum(std::string &buf, long v)
{
  char tmp[24]; int n = 0;
  unsigned long u = v < 0 ? 0ul - (unsigned long)v : (unsigned long)v;
  do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
  if (v < 0) buf.push_back('-');
  while (n) buf.push_back(tmp[--n]);
}

}  // namespace

// lines [b, e) numbered from `first`, cut at line ends into one piece per thread and parsed side by side; the regions up to the first
// line the loop cannot take
static void LinkParseText(char *b, char *e, long first, LinkColumns *col)
{
  const size_t bytes = (size_t)(e - b);
  const int T = std::max(1, std::min<int>(gtxhost::WorkerThreads(), (int)(bytes / (1u << 20)) + 1));
  struct Piece { char *b, *e; long lines = 0, first = 0; LinkColumns out; };
  std::vector<Piece> pc((size_t)T);
  for (int t = 0; t < T; t++) {
    char *pb = t == 0 ? b : pc[t - 1].e, *pe = t + 1 == T ? e : b + bytes * (size_t)(t + 1) / (size_t)T;
    if (pe < pb) pe = pb;
    while (pe < e && pe > b && pe[-1] != '\n') pe++;
    pc[t].b = pb; pc[t].e = pe;
  }
  gtxhost::ParallelFor(T, [&](int t) { pc[t].lines = gtxhost::CountNewlines(pc[t].b, pc[t].e); });
  long at = first;
  for (auto &p : pc) { p.first = at; at += p.lines; p.out.want_score = col->want_score; p.out.front_of_multi = col->front_of_multi; }
  gtxhost::ParallelFor(T, [&](int t) { LinkParsePiece(pc[t].b, pc[t].e, pc[t].first, &pc[t].out); });
  for (auto &p : pc) {
    col->append(p.out);
    if (p.out.why != LinkColumns::NONE) {
      col->why = p.out.why; col->stop_line = p.out.stop_line; col->stop_msg = p.out.stop_msg; col->stop_prefix = p.out.stop_prefix;
      col->stop_chrom = p.out.stop_chrom; col->stop_strand = p.out.stop_strand; col->stop_start = p.out.stop_start;
      break;
    }
  }
}

// items [0, n) formatted side by side in chunks and written to stdout in order
static void PrintInChunks(size_t n, const std::function<void(std::string &, size_t)> &put)
{
  StdoutIsOurs();
  const size_t per = 1u << 16, n_chunks = (n + per - 1) / per;
  const size_t wave = (size_t)std::max(1, gtxhost::WorkerThreads());
  std::vector<std::string> bufs(wave);
  for (size_t c0 = 0; c0 < n_chunks; c0 += wave) {
    const int m = (int)std::min(wave, n_chunks - c0);
    gtxhost::ParallelFor(m, [&](int t) {
      std::string &buf = bufs[(size_t)t];
      buf.clear();
      const size_t k0 = (c0 + (size_t)t) * per, k1 = std::min(n, k0 + per);
      for (size_t k = k0; k < k1; k++) put(buf, k);
    });
    for (int t = 0; t < m; t++) fwrite(bufs[(size_t)t].data(), 1, bufs[(size_t)t].size(), stdout);
  }
}

// the current region's line, then the rest of the stream, as one text of complete lines in col->text; returns the first line's number
static long int LinkReadStream(GenomicRegionSet *set, LinkColumns *col)
{
  std::string first; long int first_no = 0;
  LineSource *ls = set->DetachStream(&first, &first_no);
  col->text.assign(first.begin(), first.end()); col->text.push_back('\n');
  std::vector<char> block; long bl = 0; size_t got;
  while ((got = ls->NextBlock(block, (size_t)64 << 20, &bl)) > 0) {
    ls->AdvanceLines(gtxhost::CountNewlines(block.data(), block.data() + got));
    col->text.insert(col->text.end(), block.begin(), block.begin() + got);
  }
  return first_no;
}

// the packed triples of the columns: class = the chromosome's strcmp rank among `names` (filled here, sorted), with the strand below it
// when the set is sorted by strand
static void LinkPack(const LinkColumns &col, bool sorted_by_strand, std::vector<int32_t> *tri_out, std::vector<const char *> *names_out)
{
  const size_t n = col.size();
  std::vector<int32_t> &tri = *tri_out;
  std::vector<const char *> &names = *names_out;
  tri.resize(3 * n); names.clear();
  for (size_t k = 0; k < n; k++) if (k == 0 || (col.chrom[k] != col.chrom[k - 1] && strcmp(col.chrom[k], col.chrom[k - 1]) != 0)) names.push_back(col.chrom[k]);
  std::sort(names.begin(), names.end(), [](const char *a, const char *b) { return strcmp(a, b) < 0; });
  names.erase(std::unique(names.begin(), names.end(), [](const char *a, const char *b) { return strcmp(a, b) == 0; }), names.end());
  auto rank_of = [&](const char *c) { return (int32_t)(std::lower_bound(names.begin(), names.end(), c, [](const char *a, const char *b) { return strcmp(a, b) < 0; }) - names.begin()); };
  const int P = std::max(1, std::min<int>(gtxhost::WorkerThreads(), (int)(n >> 18) + 1));
  gtxhost::ParallelFor(P, [&](int t) {
    const size_t b = n * (size_t)t / (size_t)P, e = n * (size_t)(t + 1) / (size_t)P;
    const char *last = NULL; int32_t last_rank = 0;
    for (size_t k = b; k < e; k++) {
      if (!last || (col.chrom[k] != last && strcmp(col.chrom[k], last) != 0)) { last = col.chrom[k]; last_rank = rank_of(last); }
      tri[3 * k] = sorted_by_strand ? 2 * last_rank + (col.strand[k] == '-' ? 1 : 0) : last_rank;
      tri[3 * k + 1] = (int32_t)col.start[k]; tri[3 * k + 2] = (int32_t)col.stop[k];
    }
  });
}

// The text path of link (no label function: the labels are not needed): the file's text goes to the device block by block and is
// tokenised there (gtx_link_add_text); a block the tokenizer hands back is parsed here and its regions follow the others
// (gtx_link_add); the groups come back as head ordinal, stop and the head's (chromosome, strand, start).  The chromosome table
// comes from a first pass over the first token of every line.  A multi-interval line ends the input with its front interval as
// a last region, so that the device's order check says whether Next's order error or the interval error is the line's.
static void LinkOnDevice(char *tb, char *te, long first_no, bool sorted_by_strand, long int max_difference, bool trace)
{
  size_t target = (size_t)64 << 20;
  if (getenv("GTX_PACK_BLOCK_MB") && atol(getenv("GTX_PACK_BLOCK_MB")) > 0) target = (size_t)atol(getenv("GTX_PACK_BLOCK_MB")) << 20;
  if (getenv("GTX_LINK_BLOCK_BYTES") && atol(getenv("GTX_LINK_BLOCK_BYTES")) > 0) target = (size_t)atol(getenv("GTX_LINK_BLOCK_BYTES"));   // (tests: several blocks of a small file)
  struct Blk { char *b, *e; long lines = 0, first = 0; std::vector<std::string> names; };
  std::vector<Blk> blk;
  for (char *q = tb; q < te;) {
    char *e = (size_t)(te - q) <= target ? te : q + target;
    while (e < te && e[-1] != '\n') e++;
    Blk x; x.b = q; x.e = e; blk.push_back(x);
    q = e;
  }
  // first pass: lines per block, and the first token of every line (blanks in front skipped; it ends at a TAB or a blank)
  gtxhost::ParallelFor((int)blk.size(), [&](int t) {
    Blk &x = blk[(size_t)t];
    const char *last = NULL; size_t last_len = 0;
    for (char *q = x.b; q < x.e;) {
      char *nl = (char *)memchr(q, '\n', (size_t)(x.e - q));
      if (!nl) break;
      x.lines++;
      const char *k = q; while (k < nl && *k == ' ') k++;
      const char *k1 = k; while (k1 < nl && *k1 != '\t' && *k1 != ' ') k1++;
      const size_t len = (size_t)(k1 - k);
      if (!last || len != last_len || memcmp(last, k, len) != 0) { x.names.push_back(std::string(k, len)); last = k; last_len = len; }
      q = nl + 1;
    }
    std::sort(x.names.begin(), x.names.end()); x.names.erase(std::unique(x.names.begin(), x.names.end()), x.names.end());
  });
  std::vector<std::string> names;
  long total = 0, at = first_no;
  for (auto &x : blk) { names.insert(names.end(), x.names.begin(), x.names.end()); x.first = at; at += x.lines; total += x.lines; }
  std::sort(names.begin(), names.end(), [](const std::string &a, const std::string &b) { return strcmp(a.c_str(), b.c_str()) < 0; });
  names.erase(std::unique(names.begin(), names.end()), names.end());
  names.erase(std::remove_if(names.begin(), names.end(), [](const std::string &a) { return a.empty() || a.size() >= 4096; }), names.end());
  std::vector<const char *> name_ptr; for (auto &nm : names) name_ptr.push_back(nm.c_str());
  auto rank_of = [&](const char *c) -> int32_t {
    auto it = std::lower_bound(names.begin(), names.end(), c, [](const std::string &a, const char *b) { return strcmp(a.c_str(), b) < 0; });
    return it != names.end() && strcmp(it->c_str(), c) == 0 ? (int32_t)(it - names.begin()) : -1;
  };
  Mark("link: chromosome table made");

  gtx_group *grp = Devices();
  gtx_ctx *ctx = gtx_group_ctx(grp, 0);
  auto chk = [&](int rc) { if (rc != GTX_OK) { fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, gtx_last_error(ctx)); exit(1); } };
  gtx_text_rules rules; memset(&rules, 0, sizeof rules);
  rules.chrom_names = name_ptr.data(); rules.n_chrom = (int32_t)name_ptr.size(); rules.strand_aware = 1; rules.max_label_value = 1; rules.prev_strand = '+';
  chk(gtx_link_text_begin(ctx, rules.n_chrom, sorted_by_strand ? 1 : 0, (int64_t)total + 1));

  // where the regions of a block begin, and the lines they stand on (a block tokenised on the device: line = first + ordinal)
  struct Seg { size_t region0; long first; std::vector<long> lines; bool host; };
  std::vector<Seg> segs;
  size_t n = 0, on_device = 0, handed_back = 0;
  LinkColumns::Stop why = LinkColumns::NONE; long stop_line = 0; std::string stop_msg; bool stop_prefix = true, sentinel = false;
  for (auto &x : blk) {
    if (x.lines == 0) continue;
    int needs_host = 0;
    chk(gtx_link_add_text(ctx, x.b, (size_t)(x.e - x.b), (int64_t)x.lines, &rules, &needs_host));
    Seg sg; sg.region0 = n; sg.first = x.first; sg.host = needs_host != 0;
    if (!needs_host) { on_device++; n += (size_t)x.lines; segs.push_back(std::move(sg)); continue; }
    handed_back++;
    LinkColumns col;
    LinkParseText(x.b, x.e, x.first, &col);
    std::vector<int32_t> tri(3 * (col.size() + 1)); std::vector<uint8_t> minus(col.size() + 1);
    size_t m = col.size();
    for (size_t k = 0; k < m; k++) {
      const int32_t r = rank_of(col.chrom[k]);
      if (r < 0) { fflush(stdout); fprintf(stderr, "\nError: Line %ld: chromosome name outside the table of the first pass!\n", col.line[k]); exit(1); }
      minus[k] = col.strand[k] == '-';
      tri[3 * k] = sorted_by_strand ? 2 * r + minus[k] : r; tri[3 * k + 1] = (int32_t)col.start[k]; tri[3 * k + 2] = (int32_t)col.stop[k];
    }
    sg.lines = col.line;
    if (col.why == LinkColumns::MULTI) {
      const int32_t r = rank_of(col.stop_chrom);
      if (r >= 0 && col.stop_start >= -(long)INT_MAX && col.stop_start <= (long)INT_MAX) {
        minus[m] = col.stop_strand == '-';
        tri[3 * m] = sorted_by_strand ? 2 * r + minus[m] : r; tri[3 * m + 1] = tri[3 * m + 2] = (int32_t)col.stop_start;
        sg.lines.push_back(col.stop_line); m++; sentinel = true;
      }
    }
    chk(gtx_link_add(ctx, tri.data(), minus.data(), (int64_t)m));
    n += m; segs.push_back(std::move(sg));
    if (col.why != LinkColumns::NONE) { why = col.why; stop_line = col.stop_line; stop_msg = col.stop_msg; stop_prefix = col.stop_prefix; break; }
  }
  if (trace) fprintf(stderr, "[gtx text] link: %zu blocks tokenised on the device, %zu handed back to the host packer (%zu regions)\n", on_device, handed_back, n - (sentinel ? 1 : 0));
  Mark("link: input on the device");

  std::vector<uint32_t> head(std::max<size_t>(n, 1)); std::vector<int32_t> gstop(std::max<size_t>(n, 1)), key(2 * std::max<size_t>(n, 1));
  gtx_link_info info = {0, -1};
  chk(gtx_link_text_end(ctx, (int64_t)max_difference, head.data(), gstop.data(), key.data(), &info));
  Mark("link: groups computed");
  auto line_of = [&](size_t idx) -> long {
    size_t k = segs.size();
    while (k > 0 && segs[k - 1].region0 > idx) k--;
    const Seg &sg = segs[k - 1];
    return sg.host ? sg.lines[idx - sg.region0] : sg.first + (long)(idx - sg.region0);
  };
  size_t n_print = (size_t)info.n_groups;
  long err_line = 0; std::string err_msg; bool err_prefix = true;
  const std::string order_msg = std::string("input regions are not sorted (sorted-by-strand = ") + (sorted_by_strand ? "true" : "false") + ")!";
  if (info.first_unsorted >= 0) { err_line = line_of((size_t)info.first_unsorted); err_msg = order_msg; }
  else if (why == LinkColumns::MULTI && sentinel) {
    // in order: the groups closed in front of the line are all but the open one -- and but the line's own, when it heads one
    const size_t drop = (n_print > 0 && head[n_print - 1] == n - 1) ? 2 : 1;
    n_print = n_print > drop ? n_print - drop : 0;
    err_line = stop_line; err_msg = "not a single-interval region!";
  } else if (why != LinkColumns::NONE) {
    if (n_print > 0) n_print--;
    err_line = stop_line; err_msg = why == LinkColumns::MULTI ? "not a single-interval region!" : stop_msg; err_prefix = why == LinkColumns::MULTI || stop_prefix;
  }
  StdoutIsOurs();
  std::string buf; buf.reserve(8u << 20);
  for (size_t g = 0; g < n_print; g++) {
    buf.push_back('_'); buf.push_back('\t'); buf += names[(size_t)(key[2 * g] >> 1)]; buf.push_back(' '); buf.push_back((key[2 * g] & 1) ? '-' : '+'); buf.push_back(' ');
    LinkPutNum(buf, (long)key[2 * g + 1]); buf.push_back(' '); LinkPutNum(buf, (long)gstop[g]); buf.push_back('\n');
    if (buf.size() > (7u << 20)) { fwrite(buf.data(), 1, buf.size(), stdout); buf.clear(); }
  }
  if (!buf.empty()) fwrite(buf.data(), 1, buf.size(), stdout);
  Mark("link: output written");
  if (err_line) {
    if (err_prefix) DieLine(err_line, err_msg);
    fflush(stdout); fprintf(stderr, "%s\n", err_msg.c_str()); exit(1);
  }
}

void GenomicRegionSet::RunGlobalLink(bool sorted_by_strand, long int max_difference, char *label_func)
{
  if (n_regions == 0) return;
  if (format != "BED") PrintError("link takes BED regions on the MI355X path!");
  if (load_in_memory) PrintError("link streams its input on the MI355X path: open the set with load_in_memory = false!");
  const bool trace = getenv("GTX_TEXT_TRACE") != NULL;
  const int mode = strcmp(label_func, "sum") == 0 ? 1 : strcmp(label_func, "min") == 0 ? 2 : strcmp(label_func, "max") == 0 ? 3 : 0;
  const bool is_func = mode != 0, concat = !is_func && label_func[0] != 0;

  // ---- the input: the current region's line, then the rest of the stream ----
  LinkColumns col;
  const long int first_no = LinkReadStream(this, &col);
  Mark("link: input read");
  char *tb = col.text.data(), *te = tb + col.text.size();
  // Without a label function the labels are not needed: the text is tokenised on the device (files of 32 MB or more;
  // GTX_TEXT_ON_DEVICE=1: of any size, =0: never).  With one, the labels are read here anyway and the host packer takes the lines.
  const char *tod = getenv("GTX_TEXT_ON_DEVICE");
  const bool never = tod && atoi(tod) == 0;
  if (!label_func[0] && !never && ((tod && atoi(tod)) || col.text.size() >= ((size_t)32 << 20))) {
    LinkOnDevice(tb, te, first_no, sorted_by_strand, max_difference, trace);
    return;
  }
  LinkParseText(tb, te, first_no, &col);
  if (trace) fprintf(stderr, "[gtx text] link: %zu regions through the host packer%s\n", col.size(), label_func[0] && !never ? " (a label function reads the labels here)" : "");
  Mark("link: input parsed");
  const size_t n = col.size();

  // ---- classes: the chromosome's strcmp rank, with the strand below it when the set is sorted by strand ----
  std::vector<int32_t> tri;
  std::vector<const char *> names;
  LinkPack(col, sorted_by_strand, &tri, &names);

  // ---- a fold the device's int64 arithmetic reproduces bit for bit: canonical integers whose sums stay below 2^53 ----
  std::vector<int64_t> vals;
  bool device_fold = false;
  if (is_func && n > 0) {
    vals.resize(n);
    std::atomic<bool> ok(true);
    std::vector<long long> big((size_t)std::max(1, gtxhost::WorkerThreads()), 0);
    const int P = (int)big.size();
    gtxhost::ParallelFor(P, [&](int t) {
      const size_t b = n * (size_t)t / (size_t)P, e = n * (size_t)(t + 1) / (size_t)P;
      long long m = 0;
      for (size_t k = b; k < e && ok.load(std::memory_order_relaxed); k++) {
        long long v;
        if (!LinkCanonicalInteger(col.label[k], &v)) { ok = false; break; }
        vals[k] = v; m = std::max(m, v < 0 ? -v : v);
      }
      big[(size_t)t] = m;
    });
    const long long m = *std::max_element(big.begin(), big.end());
    device_fold = ok && (m == 0 || (double)m * (double)n < 9007199254740992.0);
  }

  // ---- the groups ----
  gtx_link_info info = {0, -1};
  std::vector<uint32_t> head(std::max<size_t>(n, 1)), count(std::max<size_t>(n, 1));
  std::vector<int32_t> gstop(std::max<size_t>(n, 1));
  std::vector<int64_t> gval(device_fold ? std::max<size_t>(n, 1) : 0);
  gtx_group *grp = Devices();
  if (n > 0) {
    const uint32_t flags = !device_fold ? 0u : mode == 1 ? GTX_LINK_SUM : mode == 2 ? GTX_LINK_MIN : GTX_LINK_MAX;
    const int rc = gtx_link(gtx_group_ctx(grp, 0), tri.data(), device_fold ? vals.data() : NULL, (int64_t)n, (int64_t)max_difference, flags, head.data(),
                            count.data(), gstop.data(), device_fold ? gval.data() : NULL, &info);
    if (rc != GTX_OK) { fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, gtx_last_error(gtx_group_ctx(grp, 0))); exit(1); }
  }
  Mark("link: groups computed");
  if (trace && is_func) fprintf(stderr, "[gtx text] link: labels folded on the %s\n", device_fold ? "device" : "host");

  // ---- which error ends the run, and the groups closed in front of it ----
  size_t n_print = (size_t)info.n_groups;
  long err_line = 0; std::string err_msg; bool err_prefix = true;
  const std::string order_msg = std::string("input regions are not sorted (sorted-by-strand = ") + (sorted_by_strand ? "true" : "false") + ")!";
  if (info.first_unsorted >= 0) { err_line = col.line[(size_t)info.first_unsorted]; err_msg = order_msg; }
  else if (col.why != LinkColumns::NONE) {
    if (n_print > 0) n_print--;                                                   // the group open at the offending line
    err_line = col.stop_line;
    if (col.why == LinkColumns::MULTI) {
      const bool before = n > 0 && LinkBefore(col.stop_chrom, col.stop_strand, col.stop_start, col.chrom[n - 1], col.strand[n - 1], col.start[n - 1], sorted_by_strand);
      err_msg = before ? order_msg : "not a single-interval region!";
    } else { err_msg = col.stop_msg; err_prefix = col.stop_prefix; }
  }

  // ---- print: chunks of groups formatted side by side, written in order ----
  PrintInChunks(n_print, [&](std::string &buf, size_t g) {
    char num[64];
    const size_t h = head[g], cnt = count[g];
    if (!label_func[0]) buf.push_back('_');
    else if (concat) {
      buf += col.label[h];
      for (size_t k = h + 1; k < h + cnt; k++) { buf += label_func; buf += col.label[k]; }
    } else {
      double v;
      if (device_fold) v = (double)gval[g];
      else {
        v = atof(col.label[h]);
        for (size_t k = h + 1; k < h + cnt; k++) { const double x = atof(col.label[k]); v = mode == 1 ? v + x : mode == 2 ? std::min(v, x) : std::max(v, x); }
      }
      buf.append(num, (size_t)snprintf(num, sizeof num, "%g", v));
    }
    buf.push_back('\t'); buf += col.chrom[h]; buf.push_back(' '); buf.push_back(col.strand[h]); buf.push_back(' ');
    LinkPutNum(buf, col.start[h]); buf.push_back(' '); LinkPutNum(buf, (long)gstop[g]); buf.push_back('\n');
  });
  Mark("link: output written");
  if (err_line) {
    if (err_prefix) DieLine(err_line, err_msg);
    fflush(stdout); fprintf(stderr, "%s\n", err_msg.c_str()); exit(1);
  }
}

// ---------------------------------------------------------------------------------------------------
// GenomicRegionSet::RunGlobalTest / RunGlobalCalcDistances / RunGlobalInvert (genomic_intervals.cpp:4755-4778, :4523-4542, :4576-4600)
// on the device: the neighbour passes gtx_adjacent / gtx_gaps over the set's packed triples
// ---------------------------------------------------------------------------------------------------
namespace {

// the set as columns and packed triples; total_lines = the number of the file's last complete line
struct AdjacentInput {
  LinkColumns col;
  std::vector<int32_t> tri;
  std::vector<const char *> names;
  long total_lines = 0;
  size_t size() const { return col.size(); }
};

void AdjacentRead(GenomicRegionSet *set, const char *what, bool by_strand, AdjacentInput *in)
{
  if (set->format != "BED") set->PrintError(std::string(what) + " takes BED regions on the MI355X path!");
  if (set->load_in_memory) set->PrintError(std::string(what) + " streams its input on the MI355X path: open the set with load_in_memory = false!");
  const long first_no = LinkReadStream(set, &in->col);
  char *tb = in->col.text.data(), *te = tb + in->col.text.size();
  in->total_lines = first_no - 1 + gtxhost::CountNewlines(tb, te);
  LinkParseText(tb, te, first_no, &in->col);
  LinkPack(in->col, by_strand, &in->tri, &in->names);
  Mark("adjacent: input parsed");
}

gtx_ctx *AdjacentContext() { return gtx_group_ctx(Devices(), 0); }

void AdjacentDie(gtx_ctx *ctx, int rc)
{
  fflush(stdout); fprintf(stderr, "\nError: [gtx %d] %s\n", rc, gtx_last_error(ctx)); exit(1);
}

// the error of the line the parser stopped at, after everything in front of it has been written
void AdjacentParserError(const LinkColumns &col, const char *multi_msg)
{
  if (col.why == LinkColumns::NONE) return;
  if (col.why == LinkColumns::MULTI) DieLine(col.stop_line, multi_msg);
  if (col.why == LinkColumns::UNSORTED_MULTI) DieLine(col.stop_line, "input regions must be compatible, sorted and non-overlapping!");
  if (col.stop_prefix) DieLine(col.stop_line, col.stop_msg);
  fflush(stdout); fprintf(stderr, "%s\n", col.stop_msg.c_str()); exit(1);
}

std::string AdjacentOrderMessage(bool sorted_by_strand)
{
  return std::string("input regions are not sorted (sorted-by-strand = ") + (sorted_by_strand ? "true" : "false") + ")!";
}

int AdjacentPoint(const char *op)
{
  return strcmp(op, "1") == 0 ? GTX_POINT_START : strcmp(op, "2") == 0 ? GTX_POINT_STOP : strcmp(op, "5p") == 0 ? GTX_POINT_5P : strcmp(op, "3p") == 0 ? GTX_POINT_3P : -1;
}

}  // namespace

void GenomicRegionSet::RunGlobalTest(bool sorted_by_strand)
{
  if (n_regions == 0) return;
  AdjacentInput in;
  in.col.front_of_multi = true;
  AdjacentRead(this, "test", sorted_by_strand, &in);
  gtx_adjacent_info info = {-1, 0, 0};
  gtx_ctx *ctx = AdjacentContext();
  const int rc = gtx_adjacent(ctx, in.tri.data(), NULL, (int64_t)in.size(), GTX_POINT_START, GTX_POINT_START, NULL, &info);
  if (rc != GTX_OK) AdjacentDie(ctx, rc);
  Mark("adjacent: pairs computed");
  if (info.first_unsorted >= 0) DieLine(in.col.line[(size_t)info.first_unsorted], AdjacentOrderMessage(sorted_by_strand));
  AdjacentParserError(in.col, "");
  fflush(stdout);
  fprintf(stderr, "* The file is sorted! Found %ld inclusions and %ld overlaps.\n", (long)info.n_inclusions, (long)info.n_overlaps);
}

void GenomicRegionSet::RunGlobalCalcDistances(char *op1, char *op2)
{
  if (n_regions == 0) return;
  AdjacentInput in;
  AdjacentRead(this, "gdist", true, &in);
  const LinkColumns &col = in.col;
  const size_t n = in.size();
  const int p1 = AdjacentPoint(op1), p2 = AdjacentPoint(op2);
  const bool known = p1 >= 0 && p2 >= 0;
  std::vector<uint8_t> minus(n);
  for (size_t k = 0; k < n; k++) minus[k] = col.strand[k] == '-';
  std::vector<int64_t> dist(std::max<size_t>(n, 1));
  gtx_adjacent_info info = {-1, 0, 0};
  gtx_ctx *ctx = AdjacentContext();
  const int rc = gtx_adjacent(ctx, in.tri.data(), minus.data(), (int64_t)n, known ? p1 : GTX_POINT_START, known ? p2 : GTX_POINT_START, dist.data(), &info);
  if (rc != GTX_OK) AdjacentDie(ctx, rc);
  Mark("adjacent: distances computed");
  // one line per pair (k - 1, k) in front of the first error; an unknown operation word is met at the first compatible pair (:471)
  size_t n_print = info.first_unsorted >= 0 ? (size_t)info.first_unsorted : n;
  bool unknown_met = false;
  if (!known)
    for (size_t k = 1; k < n_print; k++) if (dist[k] != INT64_MIN) { n_print = k; unknown_met = true; break; }
  PrintInChunks(n_print > 0 ? n_print - 1 : 0, [&](std::string &buf, size_t j) {
    const size_t k = j + 1;
    buf += col.label[k - 1]; buf.push_back('\t'); buf += col.label[k]; buf.push_back('\t');
    if (dist[k] == INT64_MIN) buf += "NaN"; else LinkPutNum(buf, (long)dist[k]);
    buf.push_back('\n');
  });
  Mark("adjacent: output written");
  if (unknown_met) {
    printf("%s\t%s\t", col.label[n_print - 1], col.label[n_print]);
    fflush(stdout); fprintf(stderr, "Error: unknown offset reference point operation!\n"); exit(1);
  }
  if (info.first_unsorted >= 0) DieLine(col.line[(size_t)info.first_unsorted], AdjacentOrderMessage(true));
  AdjacentParserError(col, "this operation requires single-interval regions!");
}

void GenomicRegionSet::RunGlobalInvert(StringLIntMap *bounds)
{
  if (n_regions == 0) return;
  AdjacentInput in;
  in.col.want_score = true;
  AdjacentRead(this, "inv", true, &in);
  const LinkColumns &col = in.col;
  const size_t n = in.size();
  // a bound per class: 2 * the chromosome's rank + strand
  std::vector<int64_t> size(2 * in.names.size(), -1);
  for (size_t r = 0; r < in.names.size(); r++) {
    StringLIntMap::iterator it = bounds->find(in.names[r]);
    if (it != bounds->end()) size[2 * r] = size[2 * r + 1] = it->second;
  }
  gtx_gaps_info info = {0, -1, 0};
  std::vector<uint32_t> owner; std::vector<int32_t> gstart, gstop;
  gtx_ctx *ctx = AdjacentContext();
  for (int64_t cap = (int64_t)(n / 2 + 1024); n > 0; cap = info.n_gaps) {       // (the policy of gtx_window_select: at most one repeat)
    owner.resize((size_t)cap); gstart.resize((size_t)cap); gstop.resize((size_t)cap);
    const int rc = gtx_gaps(ctx, in.tri.data(), (int64_t)n, size.data(), (int32_t)size.size(), cap, owner.data(), gstart.data(), gstop.data(), &info);
    if (rc != GTX_OK) AdjacentDie(ctx, rc);
    if (info.n_gaps <= cap) break;
  }
  Mark("adjacent: gaps computed");
  size_t n_print = (size_t)info.n_gaps;
  // The parser's stop line ended the run of the last region only if the reference got as far as looking at it: a malformed line dies
  // in Next() (:4588), and a multi-interval line that continues the run dies at :4589 -- in both cases before the trailing gap (:4596).
  if (info.first_bad < 0 && col.why != LinkColumns::NONE && n > 0) {
    const bool continues = col.why == LinkColumns::MULTI && strcmp(col.stop_chrom, col.chrom[n - 1]) == 0 && col.stop_strand == col.strand[n - 1];
    if (col.why != LinkColumns::MULTI || continues) {
      const bool head = n == 1 || in.tri[3 * (n - 1)] != in.tri[3 * (n - 2)];
      const size_t own_front = head ? col.start[n - 1] > 1 : col.start[n - 1] > col.stop[n - 2] + 1;
      size_t owned = 0;
      while (owned < n_print && owner[n_print - 1 - owned] == (uint32_t)(n - 1)) owned++;
      if (owned > own_front) n_print--;
    }
  }
  PrintInChunks(n_print, [&](std::string &buf, size_t g) {
    const size_t o = owner[g];
    buf += col.chrom[o]; buf.push_back('\t'); LinkPutNum(buf, (long)gstart[g] - 1); buf.push_back('\t'); LinkPutNum(buf, (long)gstop[g]);
    buf += "\t_\t"; LinkPutNum(buf, col.score[o] ? atol(col.score[o]) : 0); buf.push_back('\t'); buf.push_back(col.strand[o]); buf.push_back('\n');
  });
  Mark("adjacent: output written");
  if (info.first_bad >= 0) {
    const size_t b = (size_t)info.first_bad;
    if (info.bad_kind == 1) DieLine(col.line[b], AdjacentOrderMessage(true));
    // (:4585 prints the buffer's line counter: the line behind the head's, or 0 when the head is the file's last line)
    fflush(stdout);
    fprintf(stderr, "Line %ld: chromosome %s not found!\n", col.line[b] < in.total_lines ? col.line[b] + 1 : 0L, col.chrom[b]);
    exit(1);
  }
  AdjacentParserError(col, "not a single-interval region!");
}
