// gtx_host_regionops.cpp -- the line-based interval operations of genomic_regions on a streamed BED set: shift, shiftp, pos, center,
// fix and bounds (GenomicRegionSet::RunShiftPos, RunModifyPos, RunCenter, RunFix, RunBounds), win, the one that prints many lines
// per line (RunSlidingWindows), and bed and reg, which print a SAM, GFF or BED set in another format (RunConvertToBED,
// RunConvertToREG).  See genomic_intervals.h; shared pieces in gtx_host.h.
#include "gtx_host.h"

#include <algorithm>

using namespace gtx_host;

namespace {

struct RegionOp { int kind; std::string pos_word; long int a, b; StringLIntMap *bounds; };

// GenomicRegion::Union (genomic_intervals.cpp:1649-1671) on (start, stop) pairs: BED intervals share chromosome and strand
void Union(std::vector<long int> &iv)
{
  const size_t n = iv.size() / 2;
  if (n <= 1) return;
  std::vector<std::pair<long int, long int> > v(n);
  for (size_t k = 0; k < n; k++) v[k] = std::make_pair(iv[2 * k], iv[2 * k + 1]);
  std::stable_sort(v.begin(), v.end(), [](const std::pair<long int, long int> &x, const std::pair<long int, long int> &y) { return x.first < y.first; });
  iv.clear();
  long int start = v[0].first, stop = v[0].second;
  for (size_t k = 1; k < n; k++) {
    if (stop < v[k].first) { iv.push_back(start); iv.push_back(stop); start = v[k].first; stop = v[k].second; }
    else stop = std::max(stop, v[k].second);
  }
  iv.push_back(start); iv.push_back(stop);
}

// GenomicRegion::Fix (:1419-1425): the intervals with start < 1 or start > stop are removed
void Fix(std::vector<long int> &iv)
{
  size_t w = 0;
  for (size_t k = 0; k + 1 < iv.size(); k += 2)
    if (iv[k] >= 1 && iv[k] <= iv[k + 1]) { iv[w++] = iv[k]; iv[w++] = iv[k + 1]; }
  iv.resize(w);
}

}  // namespace

// GenomicRegionBED::UpdateThick (:2326-2333)
void gtx_host::UpdateThick(PairQuery &q)
{
  if (q.iv.empty()) return;
  q.thick_start = std::max(q.thick_start, q.iv.front() - 1);
  q.thick_end = std::min(q.thick_end, q.iv.back());
  if (q.thick_end <= q.thick_start) q.thick_start = q.thick_end = q.iv.front() - 1;
}

namespace {

// the operation on a region as GenomicRegionBED's members apply it (:2340-2480 over :524-568, :1280-1301); false: nothing is printed
bool Apply(const RegionOp &op, PairQuery &q)
{
  std::vector<long int> &iv = q.iv;
  const size_t n = iv.size() / 2;
  switch (op.kind) {
    case GTX_REWRITE_SHIFT: case GTX_REWRITE_SHIFTP:
      for (size_t k = 0; k < n; k++) {
        if (op.kind == GTX_REWRITE_SHIFTP && q.strand == '-') { iv[2 * k] -= op.b; iv[2 * k + 1] -= op.a; }
        else { iv[2 * k] += op.a; iv[2 * k + 1] += op.b; }
      }
      Union(iv); UpdateThick(q);
      break;
    case GTX_REWRITE_POS:
      for (size_t k = 0; k < n; k++) {
        long int &s = iv[2 * k], &e = iv[2 * k + 1];
        if (op.pos_word == "c") { const long int m = s + (e - s + 1) / 2; s = m - op.a; e = m + op.a; }
        else {
          const bool choose_start = op.pos_word == "1" || (q.strand == '+' && op.pos_word == "5p") || (q.strand == '-' && op.pos_word == "3p");
          if (choose_start) e = s + op.a; else s = e - op.a;
        }
      }
      Union(iv);                                                  // (no UpdateThick: :2441)
      break;
    case GTX_REWRITE_CENTER:
      for (size_t k = 0; k < n; k++) { const long int h = (iv[2 * k + 1] - iv[2 * k]) / 2; iv[2 * k] += h; iv[2 * k + 1] -= h; }
      UpdateThick(q);
      break;
    case GTX_REWRITE_FIX: Fix(iv); UpdateThick(q); break;
    default: {
      if (!op.bounds) return false;
      StringLIntMap::iterator it = op.bounds->find(q.chrom);
      if (it == op.bounds->end()) return false;                   // (:3959: not printed at all)
      const long int len = it->second;
      for (size_t k = 0; k < n; k++) {
        long int &s = iv[2 * k], &e = iv[2 * k + 1];
        if (s > len || e < 1 || e < s) s = e = 0;
        else if (s < 1 || e > len) { s = std::max(s, 1L); e = std::min(e, len); }
      }
      Fix(iv); UpdateThick(q);
    }
  }
  return !iv.empty();
}

}  // namespace

// GenomicRegionBED::Print (:2188-2218) of the region as it is now.  A 12-column region whose blocks overlap ends the run in the
// middle of its line, as the reference's does (:2207)
void gtx_host::Print(std::string &out, const PairQuery &q, long int n_line)
{
  const size_t at = out.size();
  PrintBed(out, q, q.iv, q.label, q.score, q.thick_start, q.thick_end);
  if (q.n_tokens != 12) return;
  for (size_t k = 1; k < q.iv.size() / 2; k++) {
    if (q.iv[2 * k] > q.iv[2 * k - 1]) continue;
    size_t cut = out.rfind('\t');                                 // in front of the block starts: "0", then k - 1 of them
    for (size_t j = 0; j < k; j++) cut = out.find_first_of(",\n", cut + 1);
    out.resize(std::max(cut, at));
    WriteOut(out); fflush(stdout);
    fprintf(stderr, "Line %lu: exons cannot overlap!\n", (unsigned long)n_line);
    exit(1);
  }
}

namespace {

// one region through the operation and out
void Render(std::string &out, const RegionOp &op, GenomicRegion *r, const std::string &raw)
{
  PairQuery q = PairQuery::From(r, raw);
  if (Apply(op, q)) Print(out, q, r->n_line);
  WriteOut(out, 1u << 22);
}

}  // namespace

// the host loop over what is left of the set, region by region with the reference's print; an input error ends it behind the
// output in front of the line
void gtx_host::HostLoop(GenomicRegionSet *set, const Renderer &render)
{
  std::string out;
  LoadError err;
  tls_load_error = &err;
  try {
    for (GenomicRegion *r = set->Get(); r != NULL; r = set->Next()) render(out, r, set->CurrentLine());
  } catch (const LoadAbort &) {}
  tls_load_error = NULL;
  WriteOut(out);
  ExitOnLoadError(err);
}

// the same for the lines of one block of text that came back from the device, with their own line numbers
void gtx_host::HostBlock(const char *text, size_t bytes, long int first_line, const Renderer &render, const std::string &format)
{
  std::string out, raw, line;
  LoadError err;
  tls_load_error = &err;
  try {
    long int no = first_line;
    for (const char *p = text, *end = text + bytes; p < end; no++) {
      const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
      if (!nl) break;
      raw.assign(p, nl); line = raw;
      if (format == "SAM") { GenomicRegionSAM r(&line[0], no); render(out, &r, raw); }
      else if (format == "GFF") { GenomicRegionGFF r(&line[0], no); render(out, &r, raw); }
      else { GenomicRegionBED r(&line[0], no); render(out, &r, raw); }
      p = nl + 1;
    }
  } catch (const LoadAbort &) {}
  tls_load_error = NULL;
  WriteOut(out);
  if (err.set) ExitOnLoadError(err);
}

bool gtx_host::OneGpuWithPool()
{
  if (gtx_group_size(Devices()) != 1) return false;
  if (g_pool_future.valid()) g_pool_future.get();
  return g_pool.buf[0] && g_pool.buf[1];
}

char *gtx_host::PinnedOut::Reserve(gtx_ctx *ctx, size_t need)
{
  if (need > cap_) {
    if (p_) gtx_host_free(ctx_, p_);
    ctx_ = ctx; cap_ = need + (need >> 3);
    p_ = (char *)gtx_host_alloc(ctx, cap_);
    if (!p_) DieGtx(ctx, GTX_E_HIP);
  }
  return p_;
}

gtx_host::PinnedOut::~PinnedOut() { if (p_) gtx_host_free(ctx_, p_); }

void gtx_host::DeviceTextLoop(GenomicRegionSet *set, const LineFamily &f, const Renderer &render)
{
  gtx_ctx *ctx = gtx_group_ctx(Devices(), 0);
  std::string first; long int first_no = 0;
  LineSource *src = set->DetachStream(&first, &first_no);
  if (first_no <= 0) return;
  ChromTable chroms;
  for (size_t k = 0; k < f.chrom_names.size(); k++) chroms.Add(f.chrom_names[k]);
  chroms.Freeze();
  PackOptions opt;
  opt.chroms = &chroms; opt.sam = f.sam; opt.gff = f.gff;
  BedPacker packer(src, opt);
  TextPump pump(packer, opt);
  long int on_device = 0, came_back = 0;
  if (f.view) *f.view = LineLoopView{&pump, &packer, &first, &came_back};
  const std::string format = f.sam ? "SAM" : f.gff ? "GFF" : "BED";
  pump.settle = [&](const TextPump::Block &b, int ticket) {
    if (f.result(ctx, ticket, b)) { came_back++; HostBlock(b.text, b.bytes, b.first_line, render, format); }
    else on_device++;
    return true;
  };
  pump.add = [&](const TextPump::Block &b, const gtx_text_rules &) { return f.add(ctx, b); };
  // the line the set's constructor has read for its format check: a block of one line
  first += '\n';
  TextPump::Block &one = pump.blk[0];
  one.text = &first[0]; one.bytes = first.size(); one.first_line = first_no; one.n_lines = 1; one.have_prev = false;
  pump.Add(0);
  pump.Run(1);
  fflush(stdout);
  if (getenv("GTX_TEXT_TRACE")) fprintf(stderr, "%s: %ld, came back: %ld\n", f.trace, on_device, came_back);
}

namespace {

// May the set's text go to the device as it is?  A streamed BED file, stdin or .gz (a regular file: of 32 MB or more, or
// GTX_TEXT_ON_DEVICE=1; never with GTX_TEXT_ON_DEVICE=0), on one GPU, amounts the device's arithmetic takes
bool TextUsable(GenomicRegionSet *set, const RegionOp &op)
{
  Devices();                                                      // (before anything is printed: without a GPU the run ends here)
  const long left = set->StreamBytesLeft();
  if (left >= 0 && left < (long)TextPolicy().threshold_bytes) return false;
  const long int lim = 1L << 62;
  return OneGpuWithPool() && op.a <= lim && op.a >= -lim && op.b <= lim && op.b >= -lim;
}

// the set's text through gtx_rewrite_text, the rewritten text to stdout (DeviceTextLoop)
void TextLoop(GenomicRegionSet *set, const RegionOp &op, const Renderer &render)
{
  // the names and lengths of bounds, in the map's (strcmp) order
  std::vector<const char *> names; std::vector<int64_t> lens;
  if (op.kind == GTX_REWRITE_BOUNDS && op.bounds)
    for (StringLIntMap::iterator it = op.bounds->begin(); it != op.bounds->end(); it++) { names.push_back(it->first.c_str()); lens.push_back(it->second); }
  gtx_rewrite_op dev; memset(&dev, 0, sizeof dev);
  dev.kind = op.kind; dev.a = op.a; dev.b = op.b;
  dev.pos_op = op.pos_word == "2" ? GTX_REWRITE_POS_2 : op.pos_word == "5p" ? GTX_REWRITE_POS_5P : op.pos_word == "3p" ? GTX_REWRITE_POS_3P : op.pos_word == "c" ? GTX_REWRITE_POS_C : GTX_REWRITE_POS_1;
  dev.chrom_names = names.empty() ? NULL : names.data(); dev.chrom_len = lens.empty() ? NULL : lens.data(); dev.n_chrom = (int32_t)names.size();
  PinnedOut out;
  LineLoopView loop;
  bool first_block = true;
  LineFamily f{"[gtx regions] blocks rewritten on the device", false, false, names, nullptr, nullptr, &loop};
  f.add = [&](gtx_ctx *ctx, const TextPump::Block &b) {
    int ticket = -1;
    // a short stream: the host loop is done before the device has the text
    const bool here = first_block && b.text != loop.first->data() && b.bytes < TextPolicy().threshold_bytes && loop.packer->SourceAtEnd();
    if (b.text != loop.first->data()) first_block = false;
    // (counted with the blocks that came back: the trace says how many blocks the loop rendered, whichever way they got to it)
    if (here) { loop.pump->SettleAll(); ++*loop.came_back; HostBlock(b.text, b.bytes, b.first_line, render); return ticket; }
    DieGtx(ctx, gtx_rewrite_text(ctx, b.text, b.bytes, b.n_lines, &dev, &ticket));
    return ticket;
  };
  f.result = [&](gtx_ctx *ctx, int ticket, const TextPump::Block &b) {
    const size_t cap = gtx_rewrite_max_bytes(b.bytes, b.n_lines);
    char *p = out.Reserve(ctx, cap);
    int redo = 0; size_t got = 0;
    DieGtx(ctx, gtx_rewrite_result(ctx, ticket, &redo, p, cap, &got, NULL));
    if (!redo && got) fwrite(p, 1, got, stdout);
    return redo != 0;
  };
  DeviceTextLoop(set, f, render);
}

void Run(GenomicRegionSet *set, const RegionOp &op)
{
  if (set->n_regions == 0) return;
  if (set->format != "BED") set->PrintError("unsupported input format!\n");
  if (set->load_in_memory) set->PrintError("the interval operations stream their input on the MI355X path: open the set with load_in_memory = false!");
  // GTX_TEXT_ON_DEVICE=0: the host loop and nothing else.  Otherwise the device is looked for whatever the input's size: without
  // one the run ends with the library's error, as every other operation's does
  const Renderer render = [&op](std::string &out, GenomicRegion *r, const std::string &raw) { Render(out, op, r, raw); };
  if (!TextPolicy().never && TextUsable(set, op)) TextLoop(set, op, render);
  else HostLoop(set, render);
}

// ---- win ---------------------------------------------------------------------------------------------------------------------
struct WindowsOp { long int step, size; bool small; };

// GenomicRegionBED::PrintWindows (:2520-2532) of a region, in arithmetic that cannot overflow: z <= STOP holds wherever a
// difference to STOP is taken, and a size below 1 never ends the loop (z + size - 1 <= STOP then)
void RenderWindows(std::string &out, const WindowsOp &op, GenomicRegion *r, const std::string &raw)
{
  if (r->I.size() != 1) r->PrintError("this operation requires single-interval regions!\n");
  const PairQuery q = PairQuery::From(r, raw);
  const long int start = q.iv[0], stop = q.iv[1];
  std::string tail;
  if (q.n_tokens >= 4) {
    tail += '\t'; tail += q.label;
    if (q.n_tokens >= 6) { char b[32]; snprintf(b, sizeof b, "\t%ld\t%c", q.score, q.strand); tail += b; }
  }
  tail += '\n';
  char num[48];
  for (long int z = start; z <= stop;) {
    const unsigned long room = (unsigned long)stop - (unsigned long)z;           // STOP - z, exact
    const bool cut = op.size >= 1 && (unsigned long)(op.size - 1) > room;        // z + size - 1 > STOP
    if (cut && !op.small) break;
    const long int e = cut ? stop : (long int)((unsigned long)z + (unsigned long)op.size - 1ul);
    out += q.chrom;
    out.append(num, (size_t)snprintf(num, sizeof num, "\t%ld\t%ld", z - 1, e));
    out += tail;
    WriteOut(out, 1u << 22);
    if ((unsigned long)op.step > room) break;                                    // the next z lies behind STOP
    z += op.step;
  }
}

}  // namespace

int gtx_host::WriteSink(void *user, const char *text, size_t bytes) { return fwrite(text, 1, bytes, (FILE *)user) == bytes ? 0 : 1; }

namespace {

// the set's text through gtx_windows_text; gtx_windows_result streams a block's windows to stdout (DeviceTextLoop)
void WindowsTextLoop(GenomicRegionSet *set, const WindowsOp &op, const Renderer &render)
{
  gtx_windows_op dev; memset(&dev, 0, sizeof dev);
  dev.win_size = op.size; dev.win_step = op.step; dev.small = op.small ? 1 : 0;
  LineFamily f{"[gtx windows] blocks expanded on the device", false, false, {}, nullptr, nullptr, NULL};
  f.add = [&](gtx_ctx *ctx, const TextPump::Block &b) {
    int ticket = -1;
    DieGtx(ctx, gtx_windows_text(ctx, b.text, b.bytes, b.n_lines, &dev, &ticket));
    return ticket;
  };
  f.result = [](gtx_ctx *ctx, int ticket, const TextPump::Block &) {
    int redo = 0;
    DieGtx(ctx, gtx_windows_result(ctx, ticket, &redo, WriteSink, stdout, NULL, NULL));
    return redo != 0;
  };
  DeviceTextLoop(set, f, render);
}

// May the set's text go to the device?  Whatever its size -- the output, not the input, decides what a run costs -- on one GPU, with
// a size and a step the device's arithmetic takes
bool WindowsUsable(const WindowsOp &op)
{
  const long int lim = 1L << 31;
  return OneGpuWithPool() && op.size >= 1 && op.size <= lim && op.step <= lim;
}

// ---- bed, reg ------------------------------------------------------------------------------------------------------------------
struct ConvertSpec { bool to_reg, compact, ucsc; std::string color; };

// GenomicRegion::PrintBEDFormat (:1256-1274) appended to out.  (The reference's "exons cannot overlap!" behind the first check
// cannot be reached: intervals that pass it do not overlap.)
void RenderBedFormat(std::string &out, GenomicRegion *r, const std::string &color, bool convert_chromosome)
{
  if (!r->IsCompatibleSortedAndNonoverlapping()) r->PrintError("region intervals must be compatible, sorted and non-overlapping for this operation!");
  char num[96];
  const GenomicInterval *a = r->I.front(), *z = r->I.back();
  if (convert_chromosome) { out += "chr"; out += strcmp(a->CHROMOSOME, "MT") == 0 ? "M" : a->CHROMOSOME; }   // PrintChromosome (:5968-5972)
  else out += a->CHROMOSOME;
  out.append(num, (size_t)snprintf(num, sizeof num, "\t%ld\t%ld\t", a->START - 1, z->STOP));
  out += r->LABEL;
  out.append(num, (size_t)snprintf(num, sizeof num, "\t%ld\t%c", 1000L, a->STRAND));
  if (!color.empty() || r->I.size() > 1) {
    out.append(num, (size_t)snprintf(num, sizeof num, "\t%ld\t%ld\t", a->START - 1, z->STOP));
    out += color.empty() ? "0" : color;
  }
  if (r->I.size() > 1) {
    out.append(num, (size_t)snprintf(num, sizeof num, "\t%lu\t", (unsigned long)r->I.size()));
    for (size_t k = 0; k < r->I.size(); k++) out.append(num, (size_t)snprintf(num, sizeof num, "%ld%s", r->I[k]->STOP - r->I[k]->START + 1, k + 1 == r->I.size() ? "" : ","));
    out += "\t0";
    for (size_t k = 1; k < r->I.size(); k++) out.append(num, (size_t)snprintf(num, sizeof num, ",%ld", r->I[k]->START - a->START));
  }
  out += '\n';
}

// GenomicRegion::PrintREG (:961-971) appended to out: Print (:843-849) or, compact, the starts and the stops as two lists
void RenderReg(std::string &out, GenomicRegion *r, bool compact)
{
  if (r->I.empty()) return;
  char num[96];
  const size_t n = r->I.size();
  if (compact) {
    for (size_t k = 1; k < n; k++)
      if (strcmp(r->I[0]->CHROMOSOME, r->I[k]->CHROMOSOME) != 0 || r->I[0]->STRAND != r->I[k]->STRAND)
        r->PrintError("region intervals must have the same chromosome/strand to perform conversion into compact REG format!");
    out += r->LABEL; out += '\t'; out += r->I[0]->CHROMOSOME; out += ' '; out += r->I[0]->STRAND; out += ' ';
    for (size_t k = 0; k < n; k++) out.append(num, (size_t)snprintf(num, sizeof num, "%ld%c", r->I[k]->START, k + 1 == n ? ' ' : ','));
    for (size_t k = 0; k < n; k++) out.append(num, (size_t)snprintf(num, sizeof num, "%ld%s", r->I[k]->STOP, k + 1 == n ? "" : ","));
    out += '\n';
    return;
  }
  out += r->LABEL; out += '\t';
  for (size_t k = 0; k < n; k++) {
    out += r->I[k]->CHROMOSOME;
    out.append(num, (size_t)snprintf(num, sizeof num, " %c %ld %ld", r->I[k]->STRAND, r->I[k]->START, r->I[k]->STOP));
    if (k + 1 < n) out += ' ';
  }
  out += '\n';
}

// May the set's text go to the device?  Whatever its size, on one GPU, with a colour the device's constant piece holds
bool ConvertUsable(const ConvertSpec &spec)
{
  if (!OneGpuWithPool()) return false;
  int32_t max_color = 0;
  gtx_convert_limits(NULL, NULL, &max_color);
  return spec.color.size() <= (size_t)max_color;
}

// the set's text through gtx_convert_text, the printed text to stdout (DeviceTextLoop)
void ConvertTextLoop(GenomicRegionSet *set, const ConvertSpec &spec, const Renderer &render)
{
  const bool sam = set->format == "SAM", gff = set->format == "GFF";
  const uint32_t fmt = sam ? GTX_TEXT_SAM : gff ? GTX_TEXT_GFF : 0u;
  gtx_convert_op dev; memset(&dev, 0, sizeof dev);
  dev.to = spec.to_reg ? GTX_CONVERT_REG : GTX_CONVERT_BED; dev.ucsc_names = spec.ucsc ? 1 : 0; dev.color = spec.to_reg ? NULL : spec.color.c_str();
  PinnedOut out;
  LineFamily f{"[gtx convert] blocks converted on the device", sam, gff, {}, nullptr, nullptr, NULL};
  f.add = [&](gtx_ctx *ctx, const TextPump::Block &b) {
    int ticket = -1;
    DieGtx(ctx, gtx_convert_text(ctx, b.text, b.bytes, b.n_lines, &dev, fmt, &ticket));
    return ticket;
  };
  f.result = [&](gtx_ctx *ctx, int ticket, const TextPump::Block &b) {
    const size_t cap = gtx_convert_max_bytes(b.bytes, b.n_lines, &dev);
    char *p = out.Reserve(ctx, cap);
    int redo = 0; size_t got = 0;
    DieGtx(ctx, gtx_convert_result(ctx, ticket, &redo, p, cap, &got, NULL));
    if (!redo && got) fwrite(p, 1, got, stdout);
    return redo != 0;
  };
  DeviceTextLoop(set, f, render);
}

void RunConvert(GenomicRegionSet *set, const ConvertSpec &spec, const std::string &front)
{
  if (set->n_regions == 0) return;
  if (set->format != "BED" && set->format != "SAM" && set->format != "GFF") set->PrintError("unsupported input format!\n");
  if (set->load_in_memory) set->PrintError("the conversions stream their input on the MI355X path: open the set with load_in_memory = false!");
  // a single-interval region on the device; everything the reference prints in more pieces than that, and every error, in the loop
  const bool device = !TextPolicy().never && !(set->format == "BED" && !spec.to_reg) && ConvertUsable(spec);
  if (!front.empty()) { StdoutIsOurs(); fwrite(front.data(), 1, front.size(), stdout); }
  const Renderer render = [&spec](std::string &out, GenomicRegion *r, const std::string &) {
    if (spec.to_reg) RenderReg(out, r, spec.compact); else RenderBedFormat(out, r, spec.color, spec.ucsc);
    WriteOut(out, 1u << 22);
  };
  if (device) ConvertTextLoop(set, spec, render);
  else HostLoop(set, render);
}

}  // namespace

void GenomicRegion::PrintBEDFormat(char *color, bool convert_chromosome)
{
  std::string out;
  RenderBedFormat(out, this, color ? color : "", convert_chromosome);
  WriteOut(out);
}

void GenomicRegion::PrintREG(bool compact)
{
  std::string out;
  RenderReg(out, this, compact);
  WriteOut(out);
}

void GenomicRegionSet::RunConvertToBED(char *title, char *color, char *position, bool convert_chromosome)
{
  std::string front;                                              // (:3944-3945: in front of the first region of a set that has one)
  if (position && strlen(position) > 0) { front += "browser position "; front += position; front += '\n'; }
  if (title && strlen(title) > 0) { front += "track name='"; front += title; front += "' itemRgb=On visibility=1\n"; }
  RunConvert(this, ConvertSpec{false, false, convert_chromosome, color ? color : ""}, front);
}

void GenomicRegionSet::RunConvertToREG(bool compact) { RunConvert(this, ConvertSpec{true, compact, false, ""}, ""); }

void GenomicRegionSet::RunShiftPos(long int start_shift, long int stop_shift, bool strand_aware)
{
  Run(this, RegionOp{strand_aware ? GTX_REWRITE_SHIFTP : GTX_REWRITE_SHIFT, "", start_shift, stop_shift, NULL});
}

void GenomicRegionSet::RunModifyPos(const char *position_op, long int position_shift)
{
  const std::string w = position_op;
  if (w != "1" && w != "2" && w != "5p" && w != "3p" && w != "c") { fflush(stdout); fprintf(stderr, "Error: unknown operation!\n"); exit(1); }   // (:4081)
  Run(this, RegionOp{GTX_REWRITE_POS, w, position_shift, 0, NULL});
}

void GenomicRegionSet::RunCenter() { Run(this, RegionOp{GTX_REWRITE_CENTER, "", 0, 0, NULL}); }
void GenomicRegionSet::RunFix() { Run(this, RegionOp{GTX_REWRITE_FIX, "", 0, 0, NULL}); }
void GenomicRegionSet::RunBounds(StringLIntMap *bounds) { Run(this, RegionOp{GTX_REWRITE_BOUNDS, "", 0, 0, bounds}); }

void GenomicRegionSet::RunSlidingWindows(long int win_step, long int win_size, bool win_small)
{
  // (the reference's loop does not advance with a distance below 1 and never returns: nothing bounded matches it)
  if (win_step < 1) { fflush(stdout); fprintf(stderr, "Error: window distance must be at least 1!\n"); exit(1); }
  if (n_regions == 0) return;
  if (format != "BED") PrintError("unsupported input format!\n");
  if (load_in_memory) PrintError("the interval operations stream their input on the MI355X path: open the set with load_in_memory = false!");
  const WindowsOp op{win_step, win_size, win_small};
  const Renderer render = [&op](std::string &out, GenomicRegion *r, const std::string &raw) { RenderWindows(out, op, r, raw); };
  if (!TextPolicy().never && WindowsUsable(op)) WindowsTextLoop(this, op, render);
  else HostLoop(this, render);
}
