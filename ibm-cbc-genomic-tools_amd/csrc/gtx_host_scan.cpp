// gtx_host_scan.cpp -- GenomicRegionSetScanner (the window scans on the device, what is kept there, printed and filtered) and
// GenomicRegionSetIndex.  See genomic_intervals.h; shared pieces in gtx_host.h.
#include "gtx_host.h"

#include <algorithm>
#include <iostream>
#include <map>

using namespace gtx_host;

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
  // the input's text tokenised on the device where that applies (one GPU, a streamed BED input: TextOnDevice)
  TextSink text_sink;
  text_sink.usable = [&] { return one != NULL; };
  text_sink.needs_host = [&](int ticket) { int redo = 0; DieGtx(one, gtx_text_result(one, ticket, &redo)); return redo != 0; };
  text_sink.add = [&](const char *text, size_t bytes, int64_t lines, const gtx_text_rules &rules, uint32_t text_flags) {
    if (!preprocess_ok) { bad_preprocess = true; g_drain_stop = true; return -1; }
    int ticket = -1;
    DieGtx(one, gtx_scan_add_text(one, text, bytes, lines, &rules, text_flags | ((sorted_rules || TextLooksSorted(text, bytes, text_flags & (GTX_TEXT_SAM | GTX_TEXT_GFF))) ? 0u : GTX_READS_UNSORTED), &ticket));
    return ticket;
  };
  DrainSet(R, opt, device_side, [&](const PackedBatch &b) {
    if (!preprocess_ok) { bad_preprocess = true; g_drain_stop = true; return; }
    total_label_value += (long int)b.label_sum;
    if (b.tri.empty()) return;
    if (one) { DieGtx(one, gtx_scan_add(one, b.tri.data(), b.w.empty() ? NULL : b.w.data(), (int64_t)(b.tri.size() / 3), LooksSorted(b.tri, 2) ? 0u : GTX_READS_UNSORTED)); return; }
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
    if (keep_slot >= 0) DieGtx(one, gtx_scan_end_keep(one, keep_slot, &text_labels));
    else DieGtx(one, gtx_scan_end(one, (uint64_t *)values.data(), &text_labels));
    total_label_value += (long int)text_labels;
    return;
  }
  if (keep_slot >= 0) { keep_error = "windows are kept on the device on one GPU only!"; return; }
  CheckGrp(grp, gtx_group_scan(grp, tri.data(), w.empty() ? NULL : w.data(), (int64_t)(tri.size() / 3), class_len.data(), n_chrom * ns,
                               (int32_t)win_step, (int32_t)win_size, prep, rule_flags | (LooksSorted(tri, 0) ? GTX_READS_SORTED : 0u),
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
  const uint32_t order = LooksSorted(tri, 0) ? 0u : GTX_READS_UNSORTED;
  if (gtx_group_size(grp) == 1) {
    gtx_ctx *one = gtx_group_ctx(grp, 0);
    DieGtx(one, gtx_scan_begin(one, class_len.data(), n_chrom * ns, (int32_t)win_step, (int32_t)win_size, '1', GTX_ZERO_LENGTH_OK, 1, class_off.data()));
    if (n) DieGtx(one, gtx_scan_add(one, tri.data(), w.data(), n, order));
    if (keep_slot >= 0) DieGtx(one, gtx_scan_end_keep(one, keep_slot, NULL));
    else DieGtx(one, gtx_scan_end(one, (uint64_t *)values.data(), NULL));
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

// The window vectors scanners[0 .. count) kept on the device of `one` (a null scanner is skipped: d_vec stays null) and *n, the number
// of windows they all have.  False with *error set, `who` in front of it, when one is not there or they differ.
static bool KeptVectors(gtx_ctx *one, GenomicRegionSetScanner **scanners, int count, const char *who, const void **d_vec, long long *n, std::string *error)
{
  *n = -1;
  for (int f = 0; f < count; f++) {
    if (scanners[f] == NULL) continue;
    const long long nf = scanners[f]->WindowCount();
    if (!scanners[f]->KeepError().empty()) { *error = scanners[f]->KeepError(); return false; }
    void *d = NULL; int64_t kept = 0;                                // (bounds without a window: nothing was scanned, nothing is selected)
    if (nf > 0 && (scanners[f]->KeptSlot() < 0 || gtx_scan_kept(one, scanners[f]->KeptSlot(), &d, &kept) != GTX_OK || (long long)kept != nf)) {
      *error = std::string(who) + " an input's windows are not on the device!"; return false;
    }
    if (*n >= 0 && nf != *n) { *error = std::string(who) + " the inputs differ in their number of windows!"; return false; }
    *n = nf; d_vec[f] = d;
  }
  return true;
}

// The room a selector of n windows is given for its results: max(1 << 16, n / 64) windows at first.  call(cap, &kept) resizes the
// result buffers to cap rows and runs the entry; when it reports more kept than that, it is repeated once with the reported count.
template <class Call>
static int WithRoomFor(long long n, int64_t *kept, Call call)
{
  int64_t cap = std::max<int64_t>(1 << 16, n / 64);
  for (;;) {
    const int rc = call(cap, kept);
    if (rc != GTX_OK || *kept <= cap) return rc;
    cap = *kept;
  }
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
  if (!KeptVectors(one, scanners, n_tested + n_control, "[GtxSelectWindows]", d_vec, &n, error)) return false;
  for (int f = 0; f < n_tested; f++) {
    if (tables[(size_t)f].size() != (size_t)(n_control ? win_size + 1 : 1)) { *error = "[GtxSelectWindows] a table of the wrong size!"; return false; }
    tab[f] = tables[(size_t)f].data();
  }
  const size_t cols = (size_t)(n_tested + n_control);
  int64_t kept = 0;
  const int rc = WithRoomFor(n, &kept, [&](int64_t cap, int64_t *k) {
    ordinals.resize((size_t)cap); rows.resize((size_t)cap * cols);
    return gtx_window_select(one, d_vec, n_control ? d_vec + n_tested : NULL, n_tested, n, (int32_t)win_size, tab, cap, (int64_t *)ordinals.data(), rows.data(), k);
  });
  if (rc != GTX_OK) { *error = std::string("[gtx] ") + gtx_last_error(one); return false; }
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
  if (!KeptVectors(one, scanners, 3, "[GtxSelectPeakWindows]", d_vec, &n, error)) return false;
  if (n == 0) return true;
  int64_t kept = 0;
  const int rc = WithRoomFor(n, &kept, [&](int64_t cap, int64_t *k) {
    ordinals.resize((size_t)cap); rows.resize((size_t)cap * 3);
    return gtx_peak_select(one, d_vec[0], d_vec[1], d_vec[2], n, win_size, min_reads, norm ? 1 : 0, p_ratio, cap, (int64_t *)ordinals.data(), (int64_t *)rows.data(), k);
  });
  if (rc != GTX_OK) { *error = std::string("[gtx] ") + gtx_last_error(one); return false; }
  ordinals.resize((size_t)kept); rows.resize((size_t)kept * 3);
  return true;
}

long int GenomicRegionSetScanner::TotalLabelValue()
{
  if (!computed) Compute(false);
  return total_label_value;
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

// the renderer's sink: the text to a FILE
static int WriteLines(void *user, const char *text, size_t bytes) { return fwrite(text, 1, bytes, (FILE *)user) == bytes ? 0 : 1; }

bool GenomicRegionSetScanner::LinesLayoutOnDevice(gtx_ctx *one)
{
  const size_t ns = ignore_strand ? 1 : 2, nb = n_windows.size();
  std::vector<int64_t> off(nb + 1);
  std::vector<int32_t> name_off(nb + 1, 0);
  std::string blob, strand;
  for (size_t b = 0; b < nb; b++) {
    off[b] = block_offset[b];
    blob += chrom_names[b / ns]; name_off[b + 1] = (int32_t)blob.size(); strand += (b % ns) ? '-' : '+';
  }
  off[nb] = nb ? block_offset[nb - 1] + n_windows[nb - 1] : 0;
  const int rc = nb ? gtx_lines_layout(one, off.data(), (int32_t)nb, blob.data(), name_off.data(), strand.data(), win_step, win_size) : GTX_E_ARG;
  if (rc != GTX_OK && rc != GTX_E_ARG) DieGtx(one, rc);
  return rc == GTX_OK;
}

// PrintRemaining for a scanner whose windows were kept, from the first window on.  False: the windows are on the host now (a layout
// the renderer refuses, or a walk that has begun) and the host loop prints them.
bool GenomicRegionSetScanner::PrintRemainingOnDevice(FILE *out_file, long int min_value)
{
  if (!keep_error.empty()) { std::cerr << "Error: " << keep_error << "\n"; exit(1); }
  gtx_ctx *one = gtx_group_ctx(Devices(), 0);
  const long long total = WindowCount();
  if (cur_block != 0 || cur_win != 0 || (total > 0 && !LinesLayoutOnDevice(one))) {
    GtxScanLinesFallback("a layout the renderer does not take");
    BringKeptToHost();
    return false;
  }
  // a sorted scanner's input error: the windows in front of where the walk meets it, then the error
  const long long limit = halt_set ? std::min<long long>(total, block_offset[halt_block] + halt_win) : total;
  int64_t end_at = -1;
  if (total > 0 && limit > 0) {
    void *d_windows = NULL; int64_t n_kept_windows = 0;
    DieGtx(one, gtx_scan_kept(one, keep_slot, &d_windows, &n_kept_windows));
    DieGtx(one, gtx_window_lines(one, d_windows, (int64_t)total, (int64_t)limit, (int64_t)min_value, WriteLines, out_file, NULL, NULL, &end_at));
  }
  bool raise = halt_set;
  if (end_at >= 0) {                                                 // the loop stops behind that window and looks at the halt position once more
    const size_t b = (size_t)(std::upper_bound(block_offset.begin(), block_offset.end(), (long long)end_at) - block_offset.begin()) - 1;
    const long int w = (long int)(end_at - block_offset[b]) + 1;
    raise = halt_set && (b > halt_block || (b == halt_block && w >= halt_win));
  }
  cur_block = n_windows.size(); cur_win = 0;
  if (raise) { fflush(out_file); RaiseHalt(); }
  return true;
}

void GenomicRegionSetScanner::PrintRemaining(FILE *out_file, long int min_value)
{
  if (!computed) Compute(false);
  if (keep_slot >= 0 && PrintRemainingOnDevice(out_file, min_value)) return;
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
    void *d_windows = NULL; int64_t n_kept_windows = 0;
    DieGtx(one, gtx_scan_kept(one, keep_slot, &d_windows, &n_kept_windows));
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
    DieGtx(one, gtx_window_refs(one, tri.data(), (int64_t)(tri.size() / 3), class_len.data(), class_off.data(), n_chrom * ns, (int32_t)win_step, (int32_t)win_size));
    // the lines on the device too (the pair rule over what the filter kept there), unless that is switched off or the layout refused
    const bool lines = GtxScanLinesOnDevice() && LinesLayoutOnDevice(one);
    if (lines) {
      int64_t end_at = -1;
      DieGtx(one, gtx_window_filter_lines(one, d_windows, (int64_t)total, floor_value, (int64_t)limit, WriteLines, out_file, NULL, NULL, &end_at));
      ended = end_at >= 0;
    } else {
      GtxScanLinesFallback(GtxScanLinesOnDevice() ? "a layout the renderer does not take" : "switched off, or more than one GPU");
      std::vector<long long> ordinals;
      std::vector<unsigned long long> kept_values;
      int64_t kept = 0;
      DieGtx(one, WithRoomFor(total, &kept, [&](int64_t cap, int64_t *k) {
        ordinals.resize((size_t)cap); kept_values.resize((size_t)cap);
        return gtx_window_filter(one, d_windows, (int64_t)total, floor_value, cap, (int64_t *)ordinals.data(), (uint64_t *)kept_values.data(), k);
      }));
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
