// genomic_intervals.cpp -- see genomic_intervals.h.  Host side only: the region classes and region sets (ingest, iteration, error
// messages) and the host-only passes over a file; the drivers over libgtx.so (include/gtx.h) are in gtx_host_*.cpp, one per
// family, over gtx_host.h.
#include "gtx_host.h"

#include <sys/mman.h>
#include <algorithm>
#include <chrono>
#include <iostream>
#include <shared_mutex>

using namespace gtx_host;

bool _MESSAGES_ = false;

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

char *gtx_host::CopyString(const char *s) { size_t n = strlen(s) + 1; char *p = (char *)GtxRegionAlloc(n); memcpy(p, s, n); return p; }

thread_local LoadError *gtx_host::tls_load_error = NULL;

void gtx_host::DieLine(long int n_line, const std::string &msg)
{
  if (tls_load_error) { tls_load_error->set = true; tls_load_error->line = n_line; tls_load_error->msg = msg; tls_load_error->with_prefix = true; throw LoadAbort(); }
  fflush(stdout);
  fprintf(stderr, "\n");
  fprintf(stderr, "Error: Line %ld: %s\n", n_line, msg.c_str());
  exit(1);
}

void gtx_host::DiePack(const PackError &e)
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

void gtx_host::CheckGffStrands(GenomicRegionSet *set)
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
