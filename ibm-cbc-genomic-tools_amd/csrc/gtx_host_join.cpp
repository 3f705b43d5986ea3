// gtx_host_join.cpp -- the drivers over the device join under the reference's per-query loop: overlap / intersect, subset (with its
// text path), offset, annotate (with the upstream builder) and the signal bins.  See genomic_intervals.h; shared pieces in gtx_host.h.
#include "gtx_host.h"

#include <math.h>
#include <algorithm>
#include <map>
#include <set>

using namespace gtx_host;

// ---------------------------------------------------------------------------------------------------
// genomic_overlaps overlap / intersect: the device join under the reference's per-query loop
// ---------------------------------------------------------------------------------------------------
namespace {
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

}  // namespace

PairQuery PairQuery::From(GenomicRegion *q, const std::string &current_line)
{
  GenomicInterval *f = q->I.front();
  PairQuery pq;
  pq.chrom = f->CHROMOSOME; pq.strand = f->STRAND; pq.label = q->LABEL;
  pq.n_tokens = static_cast<GenomicRegionBED *>(q)->n_tokens;
  ParseTail(current_line, pq);
  for (GenomicInterval *i : q->I) { pq.iv.push_back(i->START); pq.iv.push_back(i->STOP); }
  return pq;
}

namespace {
void AppendNum(std::string &out, long int v) { char b[24]; int n = snprintf(b, sizeof b, "%ld", v); out.append(b, (size_t)n); }
}  // namespace

void gtx_host::PrintBed(std::string &out, const PairQuery &q, const std::vector<long int> &iv, const std::string &label, long int score,
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

namespace {
// the index side of the join: classes, envelopes, intervals, order keys.  A class is the chromosome's rank in strcmp order, plus the
// number of chromosomes on '-' unless -i: the numbering of Reduce, the scanners and the device tokenizer (gtx_subset_text).  It is a
// partition label: strands come from gtx_set_ref_strands and QueryBatch::qstrand, the order of a query's pairs from gtx_set_ref_order's
// key or the ordinals.  The one reader of its VALUE, the order check of gtx_join under GTX_CHECK_SORTED, is not asked for here.
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
  int ClassOf(const GenomicInterval *i) const
  {
    std::map<std::string, int>::const_iterator it = cid.find(i->CHROMOSOME);
    if (it == cid.end()) return -1;
    return it->second + (!ignore_strand && i->STRAND == '-' ? (int)cid.size() : 0);
  }
  void Chk(int rc) const { DieGtx(ctx, rc); }
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

// gtx_join_annotate of the batch into koff / kref / kval (one kept pair each); grows and runs again like JoinPairs
void JoinAnnotate(const JoinIndex &ix, const QueryBatch &qb, uint32_t flags, int32_t mode, std::vector<int64_t> &koff, std::vector<int32_t> &kref,
                  std::vector<int64_t> &kval)
{
  const int64_t n = qb.Size();
  koff.assign((size_t)n + 1, 0);
  if (kref.empty()) { kref.resize(1 << 16); kval.resize(kref.size()); }
  auto join = [&]() {
    ix.Chk(gtx_join_annotate(ix.ctx, qb.qtri.data(), n, flags, ix.n_primary, GTX_OFFSET_5P, GTX_OFFSET_3P, mode, koff.data(), kref.data(), kval.data(),
                             (int64_t)kref.size(), NULL, NULL));
  };
  join();
  if (koff[n] > (int64_t)kref.size()) { kref.resize((size_t)koff[n]); kval.resize(kref.size()); join(); }
}

// gtx_set_ref_strands: the strand of each index region's front interval
void SetRefStrands(const JoinIndex &ix)
{
  std::vector<int8_t> strand((size_t)std::max<long int>(ix.M, 1), '+');
  for (long int k = 0; k < ix.M; k++) strand[k] = ix.regs[k]->I.front()->STRAND == '-' ? '-' : '+';
  ix.Chk(gtx_set_ref_strands(ix.ctx, strand.data()));
}

}  // namespace

void gtx_host::WriteOut(std::string &out, size_t above)
{
  if (out.size() > above) { fwrite(out.data(), 1, out.size(), stdout); out.clear(); }
}

namespace {

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

}  // namespace

void gtx_host::ExitOnLoadError(const LoadError &err)
{
  fflush(stdout);
  if (!err.set) return;
  fprintf(stderr, "\n");
  if (err.with_prefix) fprintf(stderr, "Error: Line %ld: %s\n", err.line, err.msg.c_str()); else fprintf(stderr, "%s\n", err.msg.c_str());
  exit(1);
}

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
    qb.Add(ix, q);
    batch.push_back(PairQuery::From(q, QS->CurrentLine()));
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
  GenomicRegionSet *QS = ov->QuerySet;
  if (TextPolicy().never || QS->load_in_memory || QS->format != "BED" || QS->file == NULL || QS->from_stdin) return false;
  const long left = QS->StreamBytesLeft();
  if (left < (long)TextPolicy().threshold_bytes) return false;                    // (-1: stdin, .gz)
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
  PackOptions opt;
  opt.mode = ix.sorted ? gtxhost::PACK_OVERLAPS_SORTED : gtxhost::PACK_OVERLAPS_UNSORTED;
  opt.chroms = &chroms; opt.strand_aware = !ix.ignore_strand; opt.sorted_by_strand = by_strand;
  BedPacker packer(src, opt);
  long int takeover = 0, takeover_block = 0, on_device = 0, n_blocks = 0, block_no[2] = {1, 1};
  auto report = [&]() {
    if (!getenv("GTX_TEXT_TRACE")) return;
    if (takeover) fprintf(stderr, "[gtx subset] blocks selected on the device: %ld, the loop took over at block %ld (line %ld)\n", on_device, takeover_block, takeover);
    else fprintf(stderr, "[gtx subset] blocks selected on the device: %ld, none came back\n", on_device);
  };
  // the line the set's constructor has read for its format check: packed here for what it says to the block behind it (the seam's
  // key; an error of its own is the loop's to report), and a block of one line for the device
  packer.Prime(first, first_no);
  TextPump pump(packer, opt);
  {
    PackedBatch batch; PackError err;
    packer.PackPrimedText(&batch, &err);
    if (err.set) { takeover = first_no; takeover_block = 1; report(); return takeover; }
  }
  first += '\n';
  char *out = NULL; size_t out_cap = 0;
  pump.settle = [&](const TextPump::Block &b, int ticket) {             // what the block selected goes out
    if (b.bytes > out_cap) {
      if (out) gtx_host_free(ctx, out);
      out_cap = b.bytes + (b.bytes >> 3);
      out = (char *)gtx_host_alloc(ctx, out_cap);
      if (!out) ix.Chk(GTX_E_HIP);
    }
    int redo = 0; size_t got = 0;
    ix.Chk(gtx_subset_result(ctx, ticket, &redo, out, &got, NULL));
    if (takeover) return false;                                          // (a block behind the one that came back: the loop's)
    if (redo) { takeover = b.first_line; takeover_block = block_no[&b - pump.blk]; return false; }
    if (b.text != first.data()) on_device++;
    if (got) fwrite(out, 1, got, stdout);
    return true;
  };
  pump.add = [&](const TextPump::Block &b, const gtx_text_rules &rules) {
    int ticket = -1;
    if (b.text != first.data()) block_no[&b - pump.blk] = ++n_blocks;
    if (!b.seam_ok) {                                                    // a block behind a last line that could not be read: no key for the order check at the seam
      pump.SettleAll();
      if (!takeover) { takeover = b.first_line; takeover_block = n_blocks; }
      pump.stop = true;
      return ticket;
    }
    ix.Chk(gtx_subset_text(ctx, b.text, b.bytes, b.n_lines, &rules, flags, &ticket));
    return ticket;
  };
  TextPump::Block &one = pump.blk[0];
  one.text = &first[0]; one.bytes = first.size(); one.first_line = first_no; one.n_lines = 1; one.have_prev = false;
  pump.Add(0);
  pump.Run(1);
  if (out) gtx_host_free(ctx, out);
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
    qb.Add(ix, q);
    batch.push_back(PairQuery::From(q, QS->CurrentLine()));
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
      JoinAnnotate(ix, qb, flags, mode, koff, kref, kval);
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
