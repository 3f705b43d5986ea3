// gtx_host_link.cpp -- the passes of GenomicRegionSet over a sorted stream on the device: RunGlobalLink, and the neighbour passes
// RunGlobalTest, RunGlobalCalcDistances and RunGlobalInvert, which read and pack their input as link does.  See genomic_intervals.h;
// shared pieces in gtx_host.h.
#include "gtx_host.h"

#include <algorithm>

using namespace gtx_host;

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
  gtx_text_rules rules; memset(&rules, 0, sizeof rules);
  rules.chrom_names = name_ptr.data(); rules.n_chrom = (int32_t)name_ptr.size(); rules.strand_aware = 1; rules.max_label_value = 1; rules.prev_strand = '+';
  DieGtx(ctx, gtx_link_text_begin(ctx, rules.n_chrom, sorted_by_strand ? 1 : 0, (int64_t)total + 1));

  // where the regions of a block begin, and the lines they stand on (a block tokenised on the device: line = first + ordinal)
  struct Seg { size_t region0; long first; std::vector<long> lines; bool host; };
  std::vector<Seg> segs;
  size_t n = 0, on_device = 0, handed_back = 0;
  LinkColumns::Stop why = LinkColumns::NONE; long stop_line = 0; std::string stop_msg; bool stop_prefix = true, sentinel = false;
  for (auto &x : blk) {
    if (x.lines == 0) continue;
    int needs_host = 0;
    DieGtx(ctx, gtx_link_add_text(ctx, x.b, (size_t)(x.e - x.b), (int64_t)x.lines, &rules, &needs_host));
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
    DieGtx(ctx, gtx_link_add(ctx, tri.data(), minus.data(), (int64_t)m));
    n += m; segs.push_back(std::move(sg));
    if (col.why != LinkColumns::NONE) { why = col.why; stop_line = col.stop_line; stop_msg = col.stop_msg; stop_prefix = col.stop_prefix; break; }
  }
  if (trace) fprintf(stderr, "[gtx text] link: %zu blocks tokenised on the device, %zu handed back to the host packer (%zu regions)\n", on_device, handed_back, n - (sentinel ? 1 : 0));
  Mark("link: input on the device");

  std::vector<uint32_t> head(std::max<size_t>(n, 1)); std::vector<int32_t> gstop(std::max<size_t>(n, 1)), key(2 * std::max<size_t>(n, 1));
  gtx_link_info info = {0, -1};
  DieGtx(ctx, gtx_link_text_end(ctx, (int64_t)max_difference, head.data(), gstop.data(), key.data(), &info));
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
  const bool never = TextPolicy().never;
  if (!label_func[0] && !never && col.text.size() >= TextPolicy().threshold_bytes) {
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
    gtx_ctx *ctx = gtx_group_ctx(grp, 0);
    DieGtx(ctx, gtx_link(ctx, tri.data(), device_fold ? vals.data() : NULL, (int64_t)n, (int64_t)max_difference, flags, head.data(), count.data(), gstop.data(),
                         device_fold ? gval.data() : NULL, &info));
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
  DieGtx(ctx, gtx_adjacent(ctx, in.tri.data(), NULL, (int64_t)in.size(), GTX_POINT_START, GTX_POINT_START, NULL, &info));
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
  DieGtx(ctx, gtx_adjacent(ctx, in.tri.data(), minus.data(), (int64_t)n, known ? p1 : GTX_POINT_START, known ? p2 : GTX_POINT_START, dist.data(), &info));
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
  for (int64_t cap = (int64_t)(n / 2 + 1024); n > 0; cap = info.n_gaps) {       // (the policy of WithRoomFor, gtx_host_scan.cpp: at most one repeat)
    owner.resize((size_t)cap); gstart.resize((size_t)cap); gstop.resize((size_t)cap);
    DieGtx(ctx, gtx_gaps(ctx, in.tri.data(), (int64_t)n, size.data(), (int32_t)size.size(), cap, owner.data(), gstart.data(), gstop.data(), &info));
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
