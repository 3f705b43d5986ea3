// genomic_intervals.h -- the GenomicTools class API for the count / scan hot path, MI355X edition.
//
// Same class names, constructor signatures, public members and error behaviour as the reference's
// gtools/genomic_intervals.h for the classes on the path (file:line of each counterpart is given
// at the declaration), so that callers written like gtools/genomic_overlaps.cpp:408-431 or
// gtools/genomic_scans.cpp:399-436 recompile against this header unchanged.  Underneath nothing
// is shared with the reference: region sets keep their input as a line stream that is parsed in
// bulk by a thread pool into packed int32 triples (gtx_bed.h), and the reductions
// (CountIndexOverlaps, the scanners' window sums) are one call each into the C ABI of libgtx.so
// (include/gtx.h), i.e. HIP kernels on the MI355X.  There is no CPU implementation of those
// reductions here; without a GPU they fail with an error message and exit(1), like every other
// error of the reference (genomic_intervals.cpp:1001-1006).
//
// Scope: BED3..BED12 regions (BED12 blocks as multi-interval regions) and SAM
// alignments (a spliced read as a multi-interval region) and, for the reductions, GFF / GTF features, the
// reductions of count / rpkm / coverage / density and the scanners, and the per-pair iteration
// (GetQuery / GetOverlap / NextOverlap) on the host.  REG/SEQ input, the ~45 Run*/Print*
// text transforms of GenomicRegionSet and GenomicRegionSetIndex beyond the "does anything overlap"
// query of the scanners' reference filter are outside the path; the device-side pair join is the
// C ABI's gtx_join (include/gtx.h).
#ifndef GTX_GENOMIC_INTERVALS_H
#define GTX_GENOMIC_INTERVALS_H

#include <stdio.h>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace gtxhost { class LineSource; struct GtxView; }

typedef std::map<std::string, long int> StringLIntMap;          // genomic_intervals.h:41

extern bool _MESSAGES_;                                          // verbose switch (core.h; set from -v)

// Region objects of an in-memory set are built by several threads at once (GenomicRegionSet::Init); the general heap does not
// scale there (every arena growth takes the address-space lock that page faults need), so those objects, their strings and their
// interval vectors come out of per-thread blocks owned by the set.  Objects made anywhere else use the ordinary heap; `delete`
// works on both.
void *GtxRegionAlloc(size_t bytes);                               // from the calling thread's block if it has one, else operator new
void GtxRegionFree(void *p);                                      // nothing for block memory, operator delete otherwise
template <class T> struct GtxRegionAllocator {
  typedef T value_type;
  GtxRegionAllocator() {}
  template <class U> GtxRegionAllocator(const GtxRegionAllocator<U> &) {}
  T *allocate(size_t n) { return (T *)GtxRegionAlloc(n * sizeof(T)); }
  void deallocate(T *p, size_t) { GtxRegionFree(p); }
  template <class U> bool operator==(const GtxRegionAllocator<U> &) const { return true; }
  template <class U> bool operator!=(const GtxRegionAllocator<U> &) const { return false; }
};

// ---- GenomicInterval (genomic_intervals.h:91) ---------------------------------------------------------
class GenomicInterval
{
 public:
  GenomicInterval(const char *chromosome, char strand, long int start, long int stop, long int n_line = 0);
  ~GenomicInterval();
  void PrintInterval();
  void PrintInterval(FILE *file_ptr);
  size_t GetSize() { return (size_t)(STOP - START + 1); }
  int CalcDirection(GenomicInterval *i, bool sorted_by_strand);   // <0 before i, 0 overlapping, >0 after (genomic_intervals.cpp:448-459)
  bool OverlapsWith(GenomicInterval *i, bool ignore_strand);      // :624-630
  long int CalcOverlap(GenomicInterval *i, bool ignore_strand);   // :427-432

  static void *operator new(size_t n) { return GtxRegionAlloc(n); }
  static void operator delete(void *p) { GtxRegionFree(p); }

  char *CHROMOSOME;
  char STRAND;
  long int START, STOP;          // 1-based, inclusive
  long int n_line;
};

typedef std::vector<GenomicInterval *, GtxRegionAllocator<GenomicInterval *> > GenomicIntervalSet;   // genomic_intervals.h:46 (a vector of pointers there too)

// ---- GenomicRegion (genomic_intervals.h:591) / GenomicRegionBED (:1112) ------------------------------
class GenomicRegion
{
 public:
  GenomicRegion();
  virtual ~GenomicRegion();
  void PrintError(std::string error_msg);                         // "\nError: Line N: msg\n", exit(1)
  char *GetChromosome() { return I.front()->CHROMOSOME; }
  size_t GetSize(bool skip_gaps);                                 // genomic_intervals.cpp:1049-1058
  long int GetLabelValue(long int max_label_value);               // :1081-1085
  bool IsBefore(GenomicRegion *r, bool sorted_by_strand);         // :1177-1180
  bool IsCompatibleSortedAndNonoverlapping();                     // :1153-1161 (intervals of one region: same chromosome and strand, start-sorted, disjoint)
  bool OverlapsWith(GenomicRegion *r, bool ignore_strand);        // :1167-1172 (any interval pair)
  long int CalcOverlap(GenomicRegion *r, bool ignore_strand);     // :1196-1202 (sum over interval pairs)
  int CalcDirection(GenomicRegion *r, bool sorted_by_strand);     // :1225-1236 (on the envelopes)
  // :1256-1274: the region as a BED line with score 1000 -- 6 columns, 9 with a colour, 12 for several intervals (which must be
  // compatible, sorted and disjoint: an error at the region's line otherwise); convert_chromosome: "chr" in front, MT as chrM
  void PrintBEDFormat(char *color, bool convert_chromosome);
  // :961-971: "LABEL TAB chromosome strand START STOP" of every interval, or, compact, one chromosome and strand (an error when the
  // intervals differ in them) and the starts and the stops as two comma-separated lists
  void PrintREG(bool compact = false);

  static void *operator new(size_t n) { return GtxRegionAlloc(n); }
  static void operator delete(void *p) { GtxRegionFree(p); }

  long int n_line;
  char *LABEL;
  GenomicIntervalSet I;
};

class GenomicRegionBED : public GenomicRegion
{
 public:
  // parses one BED line (the line is modified); genomic_intervals.cpp:2157-2182.  A 12-column line becomes a region of several
  // intervals (its blocks, :2174-2181)
  GenomicRegionBED(char *inp, long int n_line);
  long int n_tokens;
};

class GenomicRegionSAM : public GenomicRegion
{
 public:
  // parses one SAM alignment (the line is modified); genomic_intervals.cpp:2771-2812.  A CIGAR with 'N' operations makes a region
  // of several intervals; one without any interval on the reference (no M, D, X or N of positive length) is an input error here
  GenomicRegionSAM(char *inp, long int n_line);
  ~GenomicRegionSAM();
  long int n_tokens;
  unsigned long int FLAG;
  long int MAPQ, PNEXT, TLEN;
  char *CIGAR, *RNEXT, *SEQ, *QUAL, *OPTIONAL;                    // OPTIONAL: NULL for an 11-column line
};

class GenomicRegionGFF : public GenomicRegion
{
 public:
  // parses one GFF / GTF line (the line is modified); genomic_intervals.cpp:3501-3517.  One interval, (column 1, the first byte of
  // column 7 as it stands, column 4, column 5): 1-based and inclusive as written.  LABEL is column 9, "_" for an 8-column line.
  GenomicRegionGFF(char *inp, long int n_line);
  ~GenomicRegionGFF();
  long int n_tokens;
  char *SOURCE, *FEATURE, *SCORE, *COMMENT;                       // COMMENT (column 10): NULL with fewer than 10 tokens
  char FRAME;
};

// ---- GenomicRegionSet (genomic_intervals.h:1828) ------------------------------------------------------
class GenomicRegionSet
{
 public:
  GenomicRegionSet(char *file, unsigned long int buffer_size, bool verbose, bool load_in_memory, bool hide_header = true);
  // the same from an open stream (genomic_intervals.h:1836, .cpp:3685-3696); stdin is never loaded in memory
  GenomicRegionSet(FILE *file_ptr, unsigned long int buffer_size, bool verbose, bool load_in_memory, bool hide_header = true);
  ~GenomicRegionSet();

  GenomicRegion *Get();                                           // genomic_intervals.cpp:3845-3849
  GenomicRegion *Next(bool retain_current = false);               // :3855-3867
  GenomicRegion *Next(bool sorted_by_strand, bool retain_current); // same + order check (:3874-3882)
  void Reset();
  void PrintError(std::string error_msg);                         // "\nError: msg\n", exit(1)

  // `genomic_regions link` (genomic_intervals.cpp:4605-4644): the position-sorted set merged into groups of regions whose START lies
  // within max_difference of the group's running maximum STOP, one "label TAB chromosome strand START new_stop" line per group;
  // label_func "" prints "_", min / max / sum fold atof(LABEL), anything else is a delimiter between the members' labels.  The
  // reference's output and errors (order, multi-interval region, malformed line: the earliest line wins, with the groups closed
  // before it on stdout).  MI355X path, for a streamed BED set (load_in_memory = false).  Without a label function the text goes to
  // the device block by block and is tokenised there (files of 32 MB or more; GTX_TEXT_ON_DEVICE=1: of any size, =0: never); a block
  // the tokenizer hands back is parsed here and its regions follow the others (gtx_link_text_begin .. _end, include/gtx.h).  With a
  // label function the labels are read here, so the host packer takes every line and gtx_link gets packed triples; min / max / sum
  // run on the device for canonical integer labels, otherwise here from the device's boundaries, group by group in input order.
  // GTX_TEXT_TRACE=1 reports which way the text went.  Known limit: labels that atof() reads as nan or inf are folded with
  // std::min / std::max and printed with "%g", which may differ from the reference's stream output in spelling or in which operand wins.
  void RunGlobalLink(bool sorted_by_strand, long int max_difference, char *label_func);
  // The reference's three other operations over a position-sorted stream that compare a region with the one directly in front of it
  // (genomic_intervals.cpp:4576-4600, :4523-4542, :4755-4778): `inv` (the complement inside the chromosome bounds), `gdist` (the
  // distance between successive regions) and `test` (is the file sorted; its inclusions and overlaps).  Same signatures, output and
  // errors.  MI355X path, for a streamed BED set: the lines are read by link's host parser, packed with chromosome = strcmp rank and
  // the strand folded below it (always for inv / gdist, under sorted_by_strand for test) and handed to gtx_gaps / gtx_adjacent
  // (include/gtx.h); the printing is done here in bulk.  The earliest of {malformed line, multi-interval line, the device's first
  // bad region} ends the run, with the output in front of it on stdout.  A gap prints through the BED form of PrintModified (:2310-2314)
  // with the score of the region it is printed through -- 0 for a line with fewer than 5 tokens, where the reference's is unset.
  void RunGlobalInvert(StringLIntMap *bounds);
  void RunGlobalCalcDistances(char *op1, char *op2);
  void RunGlobalTest(bool sorted_by_strand);
  // The reference's line-based interval operations `shift` / `shiftp`, `pos`, `center`, `fix` and `bounds` (genomic_intervals.cpp
  // :4133-4139, :4079-4086, :3966-3972, :4042-4048, :3954-3960 over GenomicRegionBED's members :2340-2480): every region through the
  // operation and printed again with GenomicRegionBED::Print.  Same signatures, output and errors; an operator word of RunModifyPos
  // that is none of 1, 2, 5p, 3p, c is "Error: unknown operation!".  MI355X path, for a streamed BED set (anything else is
  // "unsupported input format!").  Two paths.  The host loop, region by region: the only path for space-separated lines, BED12, 7 to
  // 11 columns, a strand spelled ".", "1" or "-1", non-canonical numbers, and every input error with its line number behind the output
  // in front of it.  The text path, for a file of 32 MB or more, stdin or a .gz file (GTX_TEXT_ON_DEVICE=1: of any size, =0: never, and
  // then no device is looked for at all) on one GPU: blocks of the text through gtx_rewrite_text (include/gtx.h), the rewritten text
  // written as it comes back, in block order.  A block that holds a line the device does not take comes back and is rendered by the
  // host loop for that block alone, with its own line numbers; the next block goes to the device again.  GTX_TEXT_TRACE=1 reports
  // "[gtx regions] blocks rewritten on the device: N, came back: K" on stderr.  A short stream (stdin or .gz that ends inside its first block
  // of less than 32 MB, GTX_TEXT_ON_DEVICE not 1) is rendered by the loop before the device has its text, and counts under K.  Amounts beyond +-2^62 take the host loop.
  void RunShiftPos(long int start_shift, long int stop_shift, bool strand_aware);
  void RunModifyPos(const char *position_op, long int position_shift);
  void RunCenter();
  void RunFix();
  void RunBounds(StringLIntMap *bounds);
  // The reference's `win` (genomic_intervals.cpp:4449-4455 over GenomicRegionBED::PrintWindows :2520-2532): every region of a streamed
  // BED set cut into sliding windows of win_size positions win_step apart, win_small keeping the windows the region's end cuts short
  // -- `bedtools makewindows`.  Same signature and output.  MI355X path: whenever a device is usable, whatever the input's size (the
  // output decides what a run costs), the text goes to the device block by block (gtx_windows_text) and the windows of a block are
  // rendered there and streamed to stdout (gtx_windows_result); a block with a line the device does not take comes back and is
  // rendered by the host loop alone.  GTX_TEXT_ON_DEVICE=0 keeps the host loop and looks for no device; sizes below 1 or above 2^31
  // and steps above 2^31 take it too.  GTX_TEXT_TRACE=1 reports "[gtx windows] blocks expanded on the device: N, came back: K".
  // win_step < 1, with which the reference's loop never ends, is refused with one error line and exit status 1.
  void RunSlidingWindows(long int win_step, long int win_size, bool win_small);
  // The reference's `bed` and `reg` (genomic_intervals.cpp:3940-3948, :4097-4103): every region of a streamed SAM, GFF / GTF or BED
  // set printed with PrintBEDFormat or PrintREG; RunConvertToBED prints "browser position P" and "track name='T' itemRgb=On
  // visibility=1" first when position / title are not empty and the set has a region.  Same signatures and output.  MI355X path:
  // whenever a device is usable the text goes to the device block by block (gtx_convert_text) and comes back as the printed lines;
  // a block with a line the device does not take -- a spliced read, BED12, a '.' strand: everything that is not a plain
  // single-interval line -- comes back and is rendered by the host loop alone, with its own line numbers and the reference's errors.
  // GTX_TEXT_ON_DEVICE=0 keeps the host loop and looks for no device; a BED set into BED lines (the generic print of a BED region,
  // not GenomicRegionBED's) and a colour longer than gtx_convert_limits' take it too.  GTX_TEXT_TRACE=1 reports "[gtx convert] blocks
  // converted on the device: N, came back: K".
  void RunConvertToBED(char *title, char *color, char *position, bool convert_chromosome);
  void RunConvertToREG(bool compact = false);
  // The reference's `split`, `connect`, `select`, `diff`, `n` and `strand` (genomic_intervals.cpp:4187-4193, :3999-4005, :4121-4127,
  // :4011-4017, :4071-4078, :4350-4358 over GenomicRegionBED::RunSplit :2502-2505, GenomicRegion::Connect :1319-1339, Select :1493-1521,
  // Diff :1345-1361, RunSize :1451-1454, ModifyStrand :1607-1620, with UpdateThick and Print) on a streamed BED set: the operations
  // that look inside a 12-column line.  Same output and errors; RunModifyStrand has no `sorted` argument (the reference's temp-file
  // merge is not offered), and a strand_op that is none of "+", "-", "r" changes nothing, as the reference's unsorted driver has it.
  // Two conventions of this build where the reference prints an unset member: a 3-column line has the label "_", a line of fewer
  // than 5 columns the score 0 (RunSplit and RunSize print them).  MI355X path: whenever a device is usable, whatever the input's
  // size, the text goes to the device block by block (gtx_blocks_text, include/gtx.h, which has the plain line) and the printed
  // lines are streamed to stdout (gtx_blocks_result); a block with a line the device does not take -- 7 to 11 columns, blanks as
  // separators, a '.' strand, overlapping or unsorted blocks, an input error -- comes back and is rendered by the host loop alone,
  // with its own line numbers.  GTX_TEXT_ON_DEVICE=0 keeps the host loop and looks for no device.  GTX_TEXT_TRACE=1 reports
  // "[gtx blocks] blocks rendered on the device: N, came back: K".
  void RunSplit(bool by_chrom_and_strand = false);
  void RunConnect();
  void RunSelect(bool first, bool last, bool from5p, bool from3p);
  void RunDiff();
  void RunSize();
  void RunModifyStrand(const char *strand_op);

  // MI355X path: hands the not yet consumed part of a streaming set (the current region's raw
  // line first) to the bulk packer.  After this call Get()/Next() report the end of the set.
  gtxhost::LineSource *DetachStream(std::string *current_line, long int *current_line_no);
  // the same for a packed region file (format "GTX"): the view and the index of the current record
  const gtxhost::GtxView *DetachPacked(long int *current_record);

  // an in-memory set of regions made by the library itself (format "REG": it has no text behind it); the set owns them
  friend GenomicRegionSet *CreateGenomicRegionSetAnnotator(GenomicRegionSet *RefRegSet, StringLIntMap *bounds, bool ignore_strand, long int upstream_max_distance,
                                                           long int upstream_min_distance, char *bin_bits);

  char *file;
  FILE *file_ptr;                                                  // the FILE* constructor's stream (NULL otherwise)
  unsigned long int buffer_size;
  bool verbose, load_in_memory, from_stdin, hide_header;
  const std::string &CurrentLine() const { return cur_raw; }      // MI355X path: the unparsed line of the current region of a streamed text set
  long int StreamBytesLeft();                     // size of a streamed regular text file, -1 otherwise (MI355X build: the device-side tokenizer's test)
  long int n_regions;
  std::string format;                                              // "BED", "SAM", "GFF", "EMPTY" or "GTX" (a packed region file, gtx_bed.h)
  GenomicRegion **R;

 private:
  explicit GenomicRegionSet(const std::vector<GenomicRegion *> &regions);
  void Init();
  void DetectFormat(const char *first_line);
  gtxhost::LineSource *src;
  gtxhost::GtxView *packed;                                        // format "GTX"
  std::vector<std::pair<void *, size_t> > blocks_;                  // memory of the region objects built in parallel (GtxRegionAlloc)
  GenomicRegion *PackedRegion(long int record);                    // region object of one record of the packed file
  GenomicRegion *CreateRegion(char *line, long int n_line);        // GenomicRegionBED, GenomicRegionSAM or GenomicRegionGFF, by the set's format
  std::string cur_raw;                                             // unparsed copy of the current line (streaming mode)
  long int r_index;
};

// ---- GenomicRegionSetOverlaps (genomic_intervals.h:2387) ----------------------------------------------
class GenomicRegionSetOverlaps
{
 public:
  GenomicRegionSetOverlaps(GenomicRegionSet *QuerySet, GenomicRegionSet *IndexSet);
  virtual ~GenomicRegionSetOverlaps();

  virtual GenomicRegion *GetQuery() = 0;
  virtual GenomicRegion *NextQuery() = 0;
  virtual GenomicRegion *GetMatch() = 0;
  virtual GenomicRegion *NextMatch() = 0;
  virtual bool Done() = 0;

  // Per-query iteration, on the host like the reference's (it hands out GenomicRegion pointers): the index regions that overlap the
  // current query after the gap / strand filter (genomic_intervals.cpp:5224-5248), and the two per-query sums over them --
  // label values (:5291-5296) and overlap lengths x label values of the INDEX regions (:5254-5263).
  GenomicRegion *GetOverlap(bool match_gaps, bool ignore_strand);
  GenomicRegion *NextOverlap(bool match_gaps, bool ignore_strand);
  unsigned long int CalcQueryCoverage(bool match_gaps, bool ignore_strand, long int max_label_value);
  unsigned long int CountQueryOverlaps(bool match_gaps, bool ignore_strand, long int max_label_value);

  // hits[k] = sum over query regions q of w_q * [q overlaps index region k], index FILE order;
  // a new[] array the caller releases (genomic_intervals.cpp:5304-5317).  Runs on the GPU.
  unsigned long int *CountIndexOverlaps(bool match_gaps, bool ignore_strand, long int max_label_value);

  // coverage[k] = sum over query regions q overlapping index region k of w_q * overlap length
  // (genomic_intervals.cpp:5269-5285); same ownership and device path as CountIndexOverlaps.
  unsigned long int *CalcIndexCoverage(bool match_gaps, bool ignore_strand, long int max_label_value);

  GenomicRegionSet *QuerySet;
  GenomicRegionSet *IndexSet;
  GenomicRegion *current_qreg;
  GenomicRegion *current_ireg;

 protected:
  // the two reductions on the device.  Which reference algorithm's input rules apply is read off the object's type: a
  // SortedGenomicRegionSetOverlaps (or a class derived from it) has the merge's, anything else the bin index's -- the class adds no
  // virtual member to the reference's five, so a subclass written against gtools/genomic_intervals.h compiles and overrides unchanged
  unsigned long int *Reduce(bool coverage, bool match_gaps, bool ignore_strand, long int max_label_value);
};

// genomic_intervals.h:2607 -- query rules of the bin-index algorithm (any order; a query with
// stop <= 0 or start > stop on a known chromosome is an error, :5740-5741)
class UnsortedGenomicRegionSetOverlaps : public GenomicRegionSetOverlaps
{
 public:
  UnsortedGenomicRegionSetOverlaps(GenomicRegionSet *QuerySet, GenomicRegionSet *IndexSet, const char *bin_bits = NULL);
  ~UnsortedGenomicRegionSetOverlaps();
  GenomicRegion *GetQuery();
  GenomicRegion *NextQuery();
  // candidates whose envelope meets the current query's, in the reference's order: bin level by bin level, bins in ascending order,
  // inside a bin the region inserted last first (genomic_intervals.cpp:5717-5764).  A host-side bin index, built at the first call.
  GenomicRegion *GetMatch();
  GenomicRegion *NextMatch();
  bool Done();
 private:
  struct MatchIndex;
  MatchIndex *match;
  std::string bin_bits_;
};

// genomic_intervals.h:2733 -- rules of the sorted merge (both sets sorted by chromosome[, strand],
// start; violations are errors, :5868, :5894)
class SortedGenomicRegionSetOverlaps : public GenomicRegionSetOverlaps
{
 public:
  SortedGenomicRegionSetOverlaps(GenomicRegionSet *QuerySet, GenomicRegionSet *IndexSet, bool sorted_by_strand);
  ~SortedGenomicRegionSetOverlaps();
  GenomicRegion *GetQuery();
  GenomicRegion *NextQuery();
  // the merge's buffer of index regions around the current query (LoadIndexBuffer :5844-5873, GetMatch :5903-5918), on the host;
  // the index set must be loaded in memory
  GenomicRegion *GetMatch();
  GenomicRegion *NextMatch();
  bool Done();
  bool sorted_by_strand;
 private:
  void LoadIndexBuffer();
  std::vector<long int> buffer_;                                   // ordinals of the buffered index regions
  size_t buffer_at_;
  long int index_at_;                                              // next index region to pull
  bool have_union_; std::string union_chrom_; char union_strand_; long int union_start_, union_stop_;
};

// ---- GenomicRegionSetIndex (genomic_intervals.h:2505) -- only what the scanners' reference filter uses ---
// "does any region of the (in-memory) set overlap this interval": per chromosome [and strand] the regions
// sorted by start with a running maximum of their stops.  The bin levels of the reference (bin_bits) are an
// implementation detail of its search and have no observable effect; NextOverlap enumeration is outside the path.
class GenomicRegionSetIndex
{
 public:
  GenomicRegionSetIndex(GenomicRegionSet *regSet, const char *bin_bits = NULL);
  ~GenomicRegionSetIndex();
  GenomicRegion *GetOverlap(GenomicInterval *i, bool match_gaps, bool ignore_strand);   // an overlapping region or NULL (:5687-5711)
  GenomicRegionSet *regSet;
 private:
  struct Impl;
  Impl *impl;
};

// ---- scanners (genomic_intervals.h:2196, 2274, 2330) ---------------------------------------------------
class GenomicRegionSetScanner
{
 public:
  GenomicRegionSetScanner(GenomicRegionSet *R, StringLIntMap *bounds, long int win_step, long int win_size, long int max_label_value,
                          bool ignore_strand, char preprocess);
  virtual ~GenomicRegionSetScanner();

  // the reference's five pure virtuals (genomic_intervals.h:2213-2217): a scanner written against it derives from this class and
  // implements them.  The two scanners of this package share one implementation, which lives in the bodies of these members (a
  // pure virtual may have one) and which their overrides call.
  virtual void PrintInterval(FILE *out_file = stdout) = 0;        // "chr strand start stop" of the current window
  virtual GenomicInterval *GetInterval() = 0;                     // heap object owned by the caller
  virtual long int Next() = 0;                                    // next window's value, -1 at the end
  virtual long int Next(GenomicRegionSet *Ref) = 0;               // ... of the next window that overlaps a region of the sorted set (:4960-4977, :5144-5163)
  virtual long int Next(GenomicRegionSetIndex *index) = 0;        // ... of the indexed set (:4982-4991, :5168-5178)
  // MI355X path: sum of GetLabelValue(max_label_value) over every region of the input, collected by the same pass that
  // fills the windows -- what the reference gets from a separate read of the file (CountGenomicRegions, :6206-6214)
  long int TotalLabelValue();
  // an input error is waiting for the Next() call that meets it (sorted scanners): TotalLabelValue() then covers the lines in front of it only
  bool InputErrorPending() { if (!computed) Compute(false); return halt_set; }
  // MI355X path: every remaining window with a value >= min_value as "value\tchr strand start stop\n" -- what a caller's
  // Next() / PrintInterval() loop prints (genomic_scans.cpp:421-428), formatted in bulk (three stdio calls per window are half a
  // second for the three million windows of a genome at -w 1000)
  // A scanner made behind KeepNextOnDevice renders them on the device (gtx_lines_layout / gtx_window_lines, the text streamed to
  // out_file), in the host loop's order of events: the windows in front of a sorted scanner's input error, then the error; a value of
  // -1 ends the output.  A layout the renderer refuses (a chromosome name beyond its limit) brings the windows to the host first.
  void PrintRemaining(FILE *out_file, long int min_value);
  // MI355X path: the same lines for the windows that overlap a region of `index` -- what a caller's Next(index) / PrintInterval()
  // loop prints (genomic_scans.cpp:411-428) -- with the filter on the device (gtx_window_refs / gtx_window_filter): the scanner was
  // made behind KeepNextOnDevice, its windows never come to the host, only the kept ones do.  The index's regions go to the device in
  // the scan's class numbering (those on chromosomes the bounds do not name take no part).  A negative min_value counts as 0; a sorted
  // scanner's input error is met where Next() meets it; a value of -1 ends the output as it ends a caller's loop.  One GPU only.
  void PrintFiltered(FILE *out_file, GenomicRegionSetIndex *index, long int min_value);
  // MI355X path: the windows of the NEXT scanner that is constructed stay in slot `slot` (0..7) of the device context instead of
  // coming to the host (gtx_scan_end_keep) -- said before the constructor because the unsorted scanner scans in its constructor, as
  // the reference's does.  TotalLabelValue() works as before; Next() and PrintRemaining() have no values to hand out and end the
  // run; the windows are read through GtxSelectWindows, GtxSelectPeakWindows or PrintFiltered.  One GPU only (KeepError() says so otherwise).
  static void KeepNextOnDevice(int slot);
  int KeptSlot() const { return keep_slot; }
  // ... and back: the kept windows come to the host after all (gtx_scan_kept_read; the slot is dropped) and Next() hands them out as if they had never been
  // kept -- for the caller that learns only after the scans (an input error waiting in one of them) that it has to walk the windows
  void BringKeptToHost();
  long long WindowCount();                                        // windows of all blocks together (computes)
  const std::string &KeepError() const { return keep_error; }
  // "chr strand start stop" of the window with this ordinal in iteration order (0-based over all blocks): what PrintInterval()
  // prints when Next() has just returned that window
  void PrintIntervalAt(FILE *out_file, long long window);

  GenomicRegionSet *R;
  StringLIntMap *bounds;
  long int win_step, win_size, max_label_value, n_win_combine;
  bool ignore_strand;
  char preprocess;

 protected:
  void Compute(bool sorted_rules);                                // runs the GPU scan over the whole input
  void ComputeMappable(const std::vector<int32_t> &class_len, const std::vector<int64_t> &class_off);   // ... for the sorted scanner's operator 'p'
  std::vector<std::string> chrom_names;                           // bounds in std::map (strcmp) order
  std::vector<long int> n_windows;                                // per (chromosome, strand) block, iteration order
  std::vector<long long> block_offset;
  std::vector<unsigned long long> values;
  size_t cur_block;
  long int cur_win;                                               // 1-based inside the block
  bool computed;
  long int total_label_value;
  // the sorted scanner streams: an error in its input is met when the region in front of the offending line is consumed, with the
  // windows before that point already handed out (genomic_intervals.cpp:4928-4957).  Compute() scans the regions in front of the
  // line and notes where the walk stops: all windows of the blocks before halt_block, halt_win windows of that block, then the error.
  bool halt_set; size_t halt_block; long int halt_win; long int halt_line; bool halt_no_prefix; std::string halt_msg;
  void RaiseHalt();
  bool LinesLayoutOnDevice(struct gtx_ctx *one);
  bool PrintRemainingOnDevice(FILE *out_file, long int min_value);   // PrintRemaining through the renderer; false: the host loop has to                         // the blocks as the line renderer's layout; false: refused
  int keep_slot;                                                  // -1: the windows come to `values`
  std::string keep_error;
};

class SortedGenomicRegionSetScanner : public GenomicRegionSetScanner
{
 public:
  SortedGenomicRegionSetScanner(GenomicRegionSet *R, StringLIntMap *bounds, long int win_step, long int win_size, long int max_label_value,
                                bool ignore_strand, char preprocess);
  virtual ~SortedGenomicRegionSetScanner();
  virtual void PrintInterval(FILE *out_file = stdout);
  virtual GenomicInterval *GetInterval();
  virtual long int Next();
  virtual long int Next(GenomicRegionSet *Ref);
  virtual long int Next(GenomicRegionSetIndex *index);
};

class UnsortedGenomicRegionSetScanner : public GenomicRegionSetScanner
{
 public:
  UnsortedGenomicRegionSetScanner(GenomicRegionSet *R, StringLIntMap *bounds, long int win_step, long int win_size, long int max_label_value,
                                  bool ignore_strand, char preprocess);
  virtual ~UnsortedGenomicRegionSetScanner();
  virtual void PrintInterval(FILE *out_file = stdout);
  virtual GenomicInterval *GetInterval();
  virtual long int Next();
  virtual long int Next(GenomicRegionSet *Ref);
  virtual long int Next(GenomicRegionSetIndex *index);
};

// genomic_overlaps overlap / intersect (gtools/genomic_overlaps.cpp:676-741) in bulk: the reference's loop
//   for (q = GetQuery(); Done() == false; q = NextQuery()) for each overlap (GetOverlap / NextOverlap) print
// with the query stream, its errors and Done() (the merge's early stop) taken from the overlaps object itself, and the pairs of
// every batch of queries from the device join (gtx_join) in the reference's iteration order.  Each pair prints the query as
// GenomicRegionBED::Print does -- with `intersect` clipped to the index region's envelope (Constrain) -- and, with merge_labels,
// the label "query:index".  bin_bits: the -B of the bin index (its order); ignored under the sorted merge.  The query set is a
// streamed BED text set; the index set is loaded in memory.
void GtxPrintPairs(GenomicRegionSetOverlaps *overlaps, bool intersect, bool match_gaps, bool ignore_strand, bool merge_labels, const char *bin_bits);

// genomic_overlaps subset (gtools/genomic_overlaps.cpp:782-800) in bulk: the test regions that overlap some index region, with
// `inverse` (-inv) those that overlap none, each printed once as GenomicRegionBED::Print does.  Two paths.  The loop, for every
// input: the reference's loop on the overlaps object -- with `inverse` it runs while there is a query, otherwise until Done(); per
// query ONE GetOverlap(match_gaps, ignore_strand) is replayed on the class layer, which is what leaves the merge's buffer, and so
// Done(), as the reference's subset does (:794-795) -- with the hits of every batch of queries from the device (gtx_query_hits).
// The text path, when the test set is a streamed uncompressed BED file of 32 MB or more (GTX_TEXT_ON_DEVICE=1: of any size, =0:
// never) on one GPU and the index set is valid and in order: blocks of the file's text through gtx_subset_text, the selected
// lines written as they come back; the first block that holds a line the device does not take (or a query outside its rank
// difference) ends that path and the loop does the rest of the file -- it reads the file again from its start, printing nothing
// before that block, so that the merge is exactly where the reference's would be.  GTX_TEXT_TRACE=1 reports the blocks selected on
// the device and the block at which the loop took over.  The index set is loaded in memory; bin_bits as for GtxPrintPairs.
void GtxPrintSubset(GenomicRegionSetOverlaps *overlaps, bool match_gaps, bool ignore_strand, bool inverse, const char *bin_bits);

// genomic_overlaps offset (gtools/genomic_overlaps.cpp:545-670) in bulk, on the overlaps object the driver built: without -S the
// index set is the reference file and every (reference region, test region) pair prints the test envelope's offsets from the
// reference region (:595-632), with skip_ref_gaps those of every test interval inside a reference interval, less the gaps
// (:634-670); under -S the merge's queries are the reference file and the index set the test file (:545-583).  The query loop,
// its errors and the merge's early stop are GtxPrintPairs'; the offsets come from the device (gtx_join_offsets).  Per-pair errors
// of the reference (a multi-interval test region, an unknown op, start offset > stop offset) end the output where it would.
// The index set is loaded in memory.
void GtxPrintOffsets(GenomicRegionSetOverlaps *overlaps, const char *op, bool skip_ref_gaps, bool fraction, bool center, bool print_labels,
                     bool match_gaps, bool ignore_strand, const char *bin_bits);

// genomic_apps profile / heatmap (gtools/genomic_apps.cpp:560-605, :826-880): for every query of the overlaps object (an
// UnsortedGenomicRegionSetOverlaps over a reference set loaded in memory and already shifted by the caller), every pair the bin
// index hands out (match_gaps = false) adds GetLabelValue(max_label_value) to the bin of the 5' offset of the query's front
// interval from the reference region; with per_ref the bins are one row of n_bins per reference region (by ordinal: the
// reference's ireg->n_line - n_ref1 when no non-region line follows the first region).  The fused device pass
// (gtx_signal_bins) takes integral weights; a fractional weight from there on, and --skip-ref-gaps throughout, take the join's
// pairs (and offsets) to the host, which bins them in the reference's order.  The reference's errors end the run where they
// would.  Returns the number of queries (n_signal_reg).
struct GtxSignalSpec {
  bool ignore_strand, skip_ref_gaps, norm_ref_len, per_ref;
  double bin_min, bin_max, max_label_value;
  long int n_bins;
};
unsigned long int GtxSignalBins(GenomicRegionSetOverlaps *overlaps, const GtxSignalSpec &spec, std::vector<double> &bins);

// The data pass of genomic_apps peakdiff (ScanReadFiles, gtools/genomic_apps.cpp:385-412) on the device: scanners[0 .. n_tested) are the
// tested inputs, scanners[n_tested .. n_tested + n_control) their controls (n_control = 0 or n_tested), all made behind KeepNextOnDevice with
// slots of their own over the same bounds and geometry; tables[f] is tested input f's critical counts (gtx_peakdiff.h: win_size + 1
// entries with controls, one without).  Returns the kept windows' ordinals in window order and, per kept window, n_tested + n_control
// counts clamped to win_size (gtx_window_select; the result buffers grow and the call is repeated when they were too small).  False
// with *error set when the scanners cannot be selected over (more than one GPU, unequal window counts).
bool GtxSelectWindows(GenomicRegionSetScanner **scanners, int n_tested, int n_control, const std::vector<std::vector<int> > &tables, long int win_size,
                      std::vector<long long> &ordinals, std::vector<int> &rows, std::string *error);

// The head of the per-window loop of genomic_scans peaks (PeakFinder, gtools/genomic_scans.cpp:304-311) on the device: signal, control and
// uniq (the mappability track; may be NULL) are scanners made behind KeepNextOnDevice with slots of their own over the same bounds and
// geometry.  Returns the ordinals of the windows with v1 >= min_reads in window order and per kept window v1, v2, v0 after clamp and
// norm (gtx_peak_select; the result buffers grow and the call is repeated when they were too small).  False with *error set when the
// scanners cannot be selected over (more than one GPU, unequal window counts, windows not on the device).
bool GtxSelectPeakWindows(GenomicRegionSetScanner *signal, GenomicRegionSetScanner *control, GenomicRegionSetScanner *uniq, long int win_size, long int min_reads,
                          bool norm, double p_ratio, std::vector<long long> &ordinals, std::vector<long long> &rows, std::string *error);

// genomic_intervals.h:2815, .cpp:6218-6297: the upstream regions of a gene set, one per region of RefRegSet (single-interval regions
// only: anything else is that region's error), labelled "upstream:LABEL" on the gene's chromosome and strand -- on '+'
// [max(start - max, 1), max(start - 1, 1)], otherwise [stop + 1, stop + max], the stop clamped to (*bounds)[chromosome] when bounds
// are given (a chromosome the map does not name is inserted with 0, as operator[] does there).  With upstream_min_distance <
// upstream_max_distance every region is then trimmed on its 5' side against the untrimmed set, same strand only, in the order the
// set's own bin index (bin_bits) hands its overlaps out under match_gaps = true and `ignore_strand`, widened back to the minimum
// when too short, and dropped when nothing is left (:6250-6294).  The result is a new in-memory set the caller deletes; RefRegSet
// is left reset.  Host work at reference-set scale: the trimming walks the class layer's bin index, no GPU is involved.  MI355X
// path: a coordinate of the result outside the packed 32-bit range is an input error at the gene's line.
GenomicRegionSet *CreateGenomicRegionSetAnnotator(GenomicRegionSet *RefRegSet, StringLIntMap *bounds, bool ignore_strand, long int upstream_max_distance,
                                                  long int upstream_min_distance, char *bin_bits);

// genomic_overlaps annotate (gtools/genomic_overlaps.cpp:310-353, PrintAnnotations :268-290) in bulk: for every test region its
// overlaps with RefRegSet in that set's bin-index order, offset with 5p, then its overlaps with UpstreamRefRegSet (NULL: none)
// in that set's, offset with 3p; under query_op "center" a pair whose centre offset is negative is skipped, under "overlap" the
// start offset is reported, any other word is the reference's error at the first pair.  Both sets go to the device as one
// reference set whose order key ranks RefRegSet's regions first, so one join (gtx_join_annotate) returns a test region's pairs in
// print order and the annotate pass leaves only the printed pairs for the host, which formats them here.  A multi-interval test
// region is an error at its line; a multi-interval region of RefRegSet (possible only without an upstream set, whose builder
// refuses it) is an error when a pair reaches it: that case takes gtx_join's pairs and walks them on the host.  Both reference
// sets are loaded in memory; the test set is streamed.
void GtxPrintAnnotations(GenomicRegionSet *TestRegSet, GenomicRegionSet *RefRegSet, GenomicRegionSet *UpstreamRefRegSet, const char *query_op,
                         bool ignore_strand, bool distance_flag, long int proximal_dist, bool print_header, const char *bin_bits);

bool GtxScanFilterOnDevice();                                  // MI355X path: may `genomic_scans counts -r` filter on the device?  One GPU, and GTX_SCAN_FILTER_ON_DEVICE is not 0
bool GtxScanLinesOnDevice();                                   // MI355X path: may `genomic_scans counts` render its output lines on the device?  One GPU, and GTX_SCAN_LINES_ON_DEVICE is not 0
void GtxScanLinesFallback(const char *why);                    // ... the lines are about to be formatted by the host loop after all: under GTX_SCAN_LINES_ON_DEVICE=2 an error that says why, and the end of the run
bool GtxPeaksOnDevice();                                       // MI355X path: may `genomic_scans peaks` select its candidate windows on the device?  One GPU, and GTX_PEAKS_ON_DEVICE is not 0
void GtxSetDevices(int n_gpus);                               // MI355X path: GPUs the reductions are spread over (--ngpu; not in the reference)
void GtxAcceptSAM(bool on);                                      // false: a SAM or GFF file is "unsupported input format!" (drivers that print query lines; default true)
bool GtxAcceptGFF(bool on);                                      // the same for GFF alone, for the sets opened from then on; returns what it was (genomic_peakdiff, genome and -r files)
void GtxMark(const char *what);                                  // GTX_TIMING=1: wall-clock mark on stderr (not in the reference)
void GtxFinish(int code);                                        // flush and leave without the teardown (see genomic_intervals.cpp)

long int CountGenomicRegions(char *reg_file, long int max_label_value);   // a host pass over the file by the unsorted reader's rules (genomic_intervals.cpp:6206-6214)
unsigned long int CalcRegSize(char *reg_file);                   // sum of the sizes of a file's regions, gaps left out (genomic_intervals.cpp:6032-6040)
unsigned long int CalcBoundSize(StringLIntMap *bounds);          // sum of the chromosome lengths (genomic_intervals.cpp:6021-6026)

// chromosome -> length from a genome region file (genomic_intervals.cpp:5997-6015)
StringLIntMap *ReadBounds(char *genome_reg_file, bool verbose = false);

#endif
