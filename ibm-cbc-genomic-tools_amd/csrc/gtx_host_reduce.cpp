// gtx_host_reduce.cpp -- GenomicRegionSetOverlaps and its two subclasses: the count / coverage reduction on the device (Reduce) and
// the per-query iteration on the host.  See genomic_intervals.h; shared pieces in gtx_host.h.
#include "gtx_host.h"

#include <algorithm>
#include <map>

using namespace gtx_host;

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
    if (!FitsPacked(i->START) || !FitsPacked(STOP))
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
        if (!FitsPacked((*b)->START) || !FitsPacked((*b)->STOP))
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
        if (!FitsPacked((*b)->START) || !FitsPacked((*b)->STOP))
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
    uint32_t flags = mode_flags | (LooksSorted(b.tri, 2) ? GTX_READS_SORTED : 0);
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
