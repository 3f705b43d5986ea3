/*
 * gtx.h -- C ABI of the MI355X interval-overlap engine (libgtx.so).
 *
 * This is the drop-in boundary for the GenomicTools hot path
 *     genomic_overlaps count / rpkm      and      genomic_scans counts.
 * The reference has no FFI layer of its own: its boundary is the C++ class API of
 * gtools/genomic_intervals.h, called by in-tree main()s.  Each entry point below therefore
 * cites the reference method whose work it replaces; the C++ classes with the reference's
 * own names (GenomicRegionSetOverlaps, ...Scanner; see csrc/genomic_intervals.h of the
 * package) are thin shims over these calls, and INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes, no C++/torch types; status-code returns: 0 = ok, <0 = error
 *     (gtx_last_error() has the text).  No exceptions cross the boundary.
 *   - regions are packed int32 triples (class_id, start, end), 1-based inclusive coordinates,
 *     exactly what GenomicRegionBED::Read produces from a BED3..BED6 line
 *     (genomic_intervals.cpp:2157-2172: start = atol(col2)+1, stop = atol(col3)).
 *     Coordinates must lie in (-2^31+2, 2^31-2) (the kernels keep +-inf sentinels beyond them).
 *   - class_id = rank of the chromosome name in strcmp order (genomic_intervals.cpp:1227), so
 *     id order == the sort order -S expects; for strand-aware runs the caller folds the strand
 *     into the id (any injective mapping works; (strand, chrom) major order keeps a
 *     position-sorted stream class-sorted).  Two regions can overlap only inside one class
 *     (genomic_intervals.cpp:624-630).  Reads whose class has no reference region -- or lies
 *     outside [0, n_classes) -- match nothing, as an unknown chromosome does in the reference
 *     (genomic_intervals.cpp:5719-5720).
 *   - one gtx_ctx per GPU and per caller thread (the reference is single-threaded and
 *     non-reentrant, genomic_intervals.cpp:5732); multi-GPU = one process per GPU, each with
 *     its own context, partial count vectors summed by the caller (RCCL all-reduce).
 *   - the library never falls back to a CPU implementation: without a usable HIP device
 *     gtx_create() fails.
 */
#ifndef GTX_H
#define GTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gtx_ctx gtx_ctx;

/* error codes */
#define GTX_OK              0
#define GTX_E_ARG          -1   /* bad argument                                         */
#define GTX_E_HIP          -2   /* HIP runtime error (text in gtx_last_error)           */
#define GTX_E_STATE        -3   /* call order (e.g. count before set_refs)              */
#define GTX_E_RANGE        -4   /* coordinate >= 2^31-1 or negative class id in refs    */

/* flags for gtx_count* / gtx_scan* */
#define GTX_READS_SORTED    1u  /* hint: reads are sorted by (class, start) -- the streaming
                                   wave-ballot kernel is used; it is exact for ANY order, only
                                   slower on unsorted input.  Without the hint the order-agnostic
                                   path runs (bucket partition + LDS counting for large batches,
                                   per-read binary search for small ones): ~13x slower than the
                                   streaming kernel on sorted reads, ~3x faster than it on
                                   shuffled ones.  Position-sorted reads whose classes interleave
                                   (strand-aware ids on a (chrom, start)-sorted stream) are best
                                   passed WITHOUT the hint, or grouped by class first.          */
#define GTX_ZERO_LENGTH_OK   4u  /* sorted-merge semantics for degenerate reads: a zero-length read
                                   (start == end+1, BED start == end) IS counted, as
                                   SortedGenomicRegionSetOverlaps does (genomic_intervals.cpp:5903-5918
                                   has no start<=stop check); only start > end+1 is reported as
                                   degenerate.  On a reference set given with GTX_REFS_KEEP_ZERO_LENGTH the
                                   call has the merge's semantics in full: an inverted read or region
                                   (start > end+1) matches by the two comparisons of CalcDirection
                                   (:1225-1236) -- q.start <= r.stop and q.stop >= r.start -- like any other;
                                   such reads are still counted in n_degenerate, for information.
                                   Scans: GTX_ZERO_LENGTH_OK selects the sorted scanner's
                                   rule (no validity test, genomic_intervals.cpp:4933-4947).       */
#define GTX_GAPS_FORMULA     8u  /* gtx_coverage*: the overlap of a matching pair is min(ends) - max(starts) + 1 without
                                   clamping at 0 -- what CalcIndexCoverage computes under match_gaps
                                   (genomic_intervals.cpp:5278); it differs from the clamped CalcOverlap (:427-432)
                                   only for pairs with an inverted interval, so it matters only together with
                                   GTX_ZERO_LENGTH_OK on a GTX_REFS_KEEP_ZERO_LENGTH reference set            */
#define GTX_READS_UNSORTED  16u  /* gtx_coverage*, gtx_scan*: hint that the reads are in no particular order -- the partition path
                                   (buckets in LDS) instead of the streaming kernel, which is exact for any order but
                                   slow for shuffled reads.  The host-buffer calls sample their input and decide by
                                   themselves; gtx_coverage_device / gtx_scan_device take the caller's word.  Results do not depend on it. */
#define GTX_CHECK_SORTED    2u  /* also verify the order the sorted merge requires
                                   (SortedGenomicRegionSetOverlaps::NextQuery,
                                   genomic_intervals.cpp:5889-5898) and report the first
                                   violation in gtx_count_info.first_unsorted.  Only the streaming
                                   kernel looks at the order of the reads, so this flag selects it
                                   whether or not GTX_READS_SORTED is given (counts stay exact for
                                   any order; unsorted input is only slower that way)          */

/* what one count/scan call observed; valid after the call's stream has been synchronised
 * (gtx_count/gtx_scan synchronise themselves; after a *_device call use gtx_sync). */
typedef struct {
  int64_t first_unsorted;    /* index of first read that sorts before its predecessor, -1 if none
                                (only with GTX_CHECK_SORTED)                                   */
  int64_t n_no_class;        /* reads whose class is outside [0,n_classes): ignored            */
  int64_t n_degenerate;      /* reads with start > end: NOT counted by the device path; the
                                caller applies the reference's rule for them (error exit in the
                                unsorted algorithm, genomic_intervals.cpp:5740-5741)           */
  int64_t first_degenerate;  /* index of the first such read, -1 if none                       */
  int64_t n_unplaced;        /* sorted-merge semantics only: inverted reads (start > end+1) beyond the
                                capacity of the side buffer (2^20) that could NOT be matched -- nonzero
                                means the result is incomplete and the caller must treat it as an error */
} gtx_count_info;

/* ---- context ---------------------------------------------------------------------------- */

/* Binds a context to one HIP device.  Fails (NULL) when no HIP device is usable. */
gtx_ctx    *gtx_create(int device_id);
void        gtx_destroy(gtx_ctx *ctx);
/* Text of the last error on this context (or of a failed gtx_create when ctx == NULL). */
const char *gtx_last_error(const gtx_ctx *ctx);
/* All later work is enqueued on this hipStream_t (NULL = the default stream). */
int         gtx_set_stream(gtx_ctx *ctx, void *hip_stream);
/* Waits for everything the context has enqueued (its stream and its host->device copy stream). */
int         gtx_sync(gtx_ctx *ctx);

/* Page-locked host memory for the host-buffer entry points (gtx_count[_add], gtx_coverage[_add], gtx_scan).
 * Those calls stream their input through the device in batches, the host->device copy of one batch under the
 * kernels of the one before.  Ordinary (pageable) buffers are first moved into page-locked staging slots by a few
 * host threads and are free again when the call returns.  Buffers from gtx_host_alloc are read by the DMA engine
 * directly -- no staging copy -- and the call returns with the copy still in flight: such a buffer must stay
 * untouched until the context's NEXT host-buffer call, gtx_*_end or gtx_sync has returned (a producer that fills
 * two of them in turn -- what the reference's streaming GenomicRegionSet::Next loop, genomic_intervals.cpp:3855-3861,
 * becomes here -- never waits). */
void       *gtx_host_alloc(gtx_ctx *ctx, size_t bytes);
void        gtx_host_free(gtx_ctx *ctx, void *p);

/* ---- index side ------------------------------------------------------------------------- */

/* Replaces the index construction of UnsortedGenomicRegionSetOverlaps
 * (genomic_intervals.cpp:5593-5675) / the IRegBuffer of SortedGenomicRegionSetOverlaps
 * (:5844-5873): takes the M single-interval reference regions in FILE order and builds the
 * device-resident rank structure (two boundary arrays sorted by (class, coordinate)).
 * Regions with start > end or end <= 0 stay in the numbering but never match, as at :5659.
 * n_classes <= 0 means "max class id + 1". */
int gtx_set_refs(gtx_ctx *ctx, const int32_t *ref_triples, int64_t n_refs, int32_t n_classes);
/* flags for gtx_set_refs_ex */
#define GTX_REFS_KEEP_ZERO_LENGTH 1u   /* sorted-merge semantics: the merge never validates index
                                          regions, so zero-length ones (start == end+1), ones with
                                          end <= 0 and inverted ones (start > end+1) all take part
                                          (the last only in calls made with GTX_ZERO_LENGTH_OK)      */
/* A region with class id -1 is a placeholder: it keeps its place in the numbering and never matches. */
int gtx_set_refs_ex(gtx_ctx *ctx, const int32_t *ref_triples, int64_t n_refs, int32_t n_classes, uint32_t flags);
int64_t gtx_n_refs(const gtx_ctx *ctx);

/* ---- genomic_overlaps count ------------------------------------------------------------- */

/* Replaces GenomicRegionSetOverlaps::CountIndexOverlaps (genomic_intervals.cpp:5304-5317,
 * decl genomic_intervals.h:2471) for single-interval regions with match_gaps = false:
 *     hits[k] = sum over reads q of w_q * [q overlaps reference k]
 * in reference FILE order, 64-bit unsigned wrap-around arithmetic like the reference's
 * `unsigned long`.  weights == NULL means w_q = 1 (--max-label-value <= 1,
 * genomic_intervals.cpp:1081-1085); otherwise weights[q] is the already clamped label value.
 * Host buffers in, host buffer out; copies + kernels + sync inside. */
int gtx_count(gtx_ctx *ctx, const int32_t *read_triples, const int32_t *weights, int64_t n_reads,
              uint32_t flags, uint64_t *hits_out /* n_refs */, gtx_count_info *info /* may be NULL */);

/* Streaming form of gtx_count for a query set that is never held in memory (the reference's
 * load_in_memory=false mode, genomic_intervals.cpp:3855-3861): begin, any number of add calls with
 * consecutive batches of the stream, end.  gtx_count(...) == begin + add + end.  Indices in `info`
 * are positions in the whole stream. */
int gtx_count_begin(gtx_ctx *ctx);
int gtx_count_add(gtx_ctx *ctx, const int32_t *read_triples, const int32_t *weights, int64_t n_reads, uint32_t flags);
int gtx_count_end(gtx_ctx *ctx, uint64_t *hits_out /* n_refs */, gtx_count_info *info /* may be NULL */);

/* Same with reads (and weights) already resident in this device's HBM and the count vector
 * left in HBM (d_hits_out: uint64[n_refs], overwritten).  Asynchronous on the context's stream.
 * This is the entry the benchmark times and the one a multi-GPU caller reduces from. */
int gtx_count_device(gtx_ctx *ctx, const void *d_read_triples, const void *d_weights, int64_t n_reads,
                     uint32_t flags, void *d_hits_out);
/* Result of the most recent *_device call (synchronises the stream). */
int gtx_last_info(gtx_ctx *ctx, gtx_count_info *info);

/* ---- count over multi-interval (BED12) regions, match_gaps = false ------------------------ */

/* CountIndexOverlaps counts a query once for an index region when GetMatch / NextMatch deliver the pair -- their envelopes
 * (first interval's start .. last interval's stop) overlap, genomic_intervals.cpp:5752 -- and GenomicRegion::OverlapsWith holds:
 * SOME interval of the one overlaps SOME interval of the other (:1167-1172, :5226-5232).  With match_gaps = true the envelope
 * alone decides, and a caller simply hands over envelopes as triples.  Without it:
 *
 * gtx_set_ref_blocks declares the intervals of the index regions given to gtx_set_refs[_ex] (whose triples must be the
 * envelopes): region k's intervals are blocks[2 * first[k]] .. blocks[2 * first[k+1] - 1] as (start, stop) pairs, sorted and
 * disjoint as IsCompatibleSortedAndNonoverlapping demands (:1153-1161; GTX_E_RANGE when starts or stops decrease).  From then
 * on every count call of the context (gtx_count*, gtx_count_device, gtx_count_add_text) takes the reads that lie in a gap of a
 * multi-interval region off that region's count again.  first == NULL: back to envelopes only.  gtx_set_refs clears it.
 *
 * gtx_count_add_regions adds multi-interval QUERIES to an open count stream (gtx_count_begin): env_triples are their
 * (class, envelope start, envelope stop), first / blocks their intervals as above; each is counted once for every index region
 * one of its intervals overlaps.  They never enter the streaming kernel (a side channel: one lane per query, candidates from
 * the index regions' envelopes in the order of their starts). */
int gtx_set_ref_blocks(gtx_ctx *ctx, const int64_t *first /* n_refs + 1, or NULL */, const int32_t *blocks);
int gtx_count_add_regions(gtx_ctx *ctx, const int32_t *env_triples, const int32_t *weights /* may be NULL */,
                          const int64_t *first /* n + 1 */, const int32_t *blocks, int64_t n);

/* ---- genomic_overlaps overlap / intersect: the overlap join ----------------------------------- */

/* The per-pair operations of the reference (genomic_overlaps overlap :706-741, intersect :676-701) walk
 * GetOverlap / NextOverlap for every query and print one line per (query, reference region) pair.  The join
 * computes all pairs of a batch of queries at once, as a CSR array: offsets[i] .. offsets[i+1] are the
 * positions of query i's pairs, each pair the ordinal (position in the set given to gtx_set_refs[_ex]) of a
 * reference region the query overlaps.  Which pairs: those count would count with the same flags -- the
 * merge's two comparisons on the envelopes (genomic_intervals.cpp:1225-1236) under the rules of the reference
 * set (gtx_set_refs_ex) and of GTX_ZERO_LENGTH_OK, then, without GTX_JOIN_GAPS, some pair of intervals
 * (:1167-1172) over the intervals of gtx_set_ref_blocks and those of multi-interval queries.
 *
 * Within a query the pairs follow a per-region order key: ascending (key[k], k).  gtx_set_ref_order sets the
 * keys (n_refs int64; NULL = the ordinal itself, the default and the order of the sorted merge, :5844-5930).
 * The bin index of UnsortedGenomicRegionSetOverlaps hands regions out level by level from the finest, bins
 * ascending within a level, last inserted first within a bin (:5655-5674, :5729-5764); a region's level and
 * bin depend on the region alone, so that order is the key (level, bin, -ordinal), e.g. its rank.
 * gtx_set_refs clears the keys.
 *
 * gtx_join: queries from host memory (triples; multi-interval queries as in gtx_count_add_regions: first /
 * blocks, NULL when every query has one interval), offsets_out (n_reads + 1) always complete, pairs_out
 * receives the first min(offsets_out[n_reads], pair_capacity) pairs.  Internally the queries travel in
 * batches and the pairs in chunks of at most gtx_set_join_buffer pairs (default 2^26): a chunk is the
 * longest run of queries that fits, a query with more pairs than that is emitted alone into a buffer of
 * its own size.  info as for gtx_count (indices are query positions; n_unplaced stays 0).
 *
 * gtx_join_device: queries (single-interval triples), offsets (int64[n_reads + 1]) and pairs (int32[pair_capacity])
 * in this device's HBM.  The offsets of all n_reads queries are written; the pairs of the longest run of
 * queries from the first whose pairs fit pair_capacity: *n_done_out of them (0 when the first query alone has
 * more), *n_pairs_out = offsets[n_reads].  Returns with the work complete. */
#define GTX_JOIN_GAPS       32u  /* gtx_join*: -gaps -- the envelopes alone decide (match_gaps = true)            */
int gtx_set_ref_order(gtx_ctx *ctx, const int64_t *key /* n_refs, or NULL = ordinal */);
int gtx_set_join_buffer(gtx_ctx *ctx, int64_t max_pairs);
int gtx_join(gtx_ctx *ctx, const int32_t *read_triples, const int64_t *first /* n + 1, or NULL */, const int32_t *blocks,
             int64_t n_reads, uint32_t flags, int64_t *offsets_out /* n_reads + 1 */, int32_t *pairs_out,
             int64_t pair_capacity, gtx_count_info *info /* may be NULL */);
int gtx_join_device(gtx_ctx *ctx, const void *d_read_triples, int64_t n_reads, uint32_t flags, void *d_offsets,
                    void *d_pairs, int64_t pair_capacity, int64_t *n_pairs_out, int64_t *n_done_out,
                    gtx_count_info *info /* may be NULL */);

/* ---- genomic_overlaps subset: hits per query ---------------------------------------------------- */

/* genomic_overlaps subset (gtools/genomic_overlaps.cpp:782-800) keeps the test regions that overlap some reference
 * region, or with -inv those that overlap none; CountQueryOverlaps (genomic_intervals.cpp:5292-5302) is the same
 * answer as a number: how many index regions GetOverlap / NextOverlap deliver for a query, each after the filter of
 * :5224-5248.  Where every other count of this library is keyed by the reference region, this one is keyed by the
 * query:
 *     hits[i] = the number of reference regions query i overlaps
 *             = offsets[i + 1] - offsets[i] of gtx_join with the same reference set, blocks and flags,
 * with the same info.  A query whose class is outside [0, n_classes) has 0.  flags: GTX_ZERO_LENGTH_OK,
 * GTX_JOIN_GAPS, GTX_CHECK_SORTED.
 *
 * The hits are the counts of the join's first pass (one walk of the envelope index per query), narrowed to 32 bits: no
 * offsets are scanned and no pair is written.  Every rule of gtx_join holds as it stands: gtx_set_ref_blocks, multi-interval
 * queries, GTX_REFS_KEEP_ZERO_LENGTH sets with inverted regions, zero-length and inverted queries under GTX_ZERO_LENGTH_OK.
 *
 * gtx_query_hits: queries from host memory as gtx_join takes them (first / blocks: NULL when every query has one
 * interval), in batches; hits_out receives n_reads values.
 * gtx_query_hits_device: single-interval triples and the hits (uint32[n_reads]) in this device's HBM.
 * Both return with the work complete. */
int gtx_query_hits(gtx_ctx *ctx, const int32_t *read_triples, const int64_t *first /* n + 1, or NULL */, const int32_t *blocks,
                   int64_t n_reads, uint32_t flags, uint32_t *hits_out /* n_reads */, gtx_count_info *info /* may be NULL */);
int gtx_query_hits_device(gtx_ctx *ctx, const void *d_read_triples, int64_t n_reads, uint32_t flags,
                          void *d_hits /* uint32[n_reads] */, gtx_count_info *info /* may be NULL */);

/* ---- genomic_overlaps offset: pair offsets on the join ----------------------------------------- */

/* genomic_overlaps offset (gtools/genomic_overlaps.cpp:545-670) prints, per (test region, reference region)
 * pair of the join, where the one lies relative to a reference point of the other: GetOffsetFrom
 * (genomic_intervals.cpp:646-667) takes the front or back interval of the point's region by op and strand
 * (2, -5p and +3p: the back one), its coordinate (GetCoordinate :465-472: 1 start, 2 stop, 5p / 3p by
 * strand), and returns {start - ref, stop - ref} of the other region's envelope, or {ref - stop, ref - start}
 * for -5p and +3p.  The point's strand decides (within a pair the strands agree unless -i, and under -i the
 * reference's is the one used).
 *
 * gtx_set_ref_strands: the strand of every reference region ('+' or '-'; NULL: all '+'), since classes carry
 * none under -i; gtx_set_refs clears it.  The front / back intervals are those of gtx_set_ref_blocks (or the
 * envelope of a single-interval region).
 *
 * gtx_join_offsets: gtx_join (same queries, flags, offsets_out, pairs_out, pair_capacity, info) plus, for each
 * pair p of the first min(pairs, pair_capacity), its entries entries_out[2 e], [2 e + 1] (start, stop offset)
 * for e in entry_offsets_out[p] .. entry_offsets_out[p + 1] (pair_capacity + 1 offsets); entries_out receives
 * the first entry_capacity entries.  Without GTX_OFFSET_SKIP_REF_GAPS a pair has one entry, its offsets; with
 * GTX_OFFSET_FROM_QUERY the query is the point (its intervals from first / blocks, its strand from
 * read_strands, NULL: all '+') and the reference region's envelope is offset -- the sorted branch, where the
 * merge's queries are the reference file.  With GTX_OFFSET_SKIP_REF_GAPS (CalcOffsetsWithoutGaps :6176-6199;
 * not with GTX_OFFSET_FROM_QUERY) a pair has one entry per (reference interval k, query interval contained in
 * it), k outer: that interval's offsets minus the gaps of the reference before interval k (after it for 2,
 * +3p and -5p); a pair whose query or reference intervals are not sorted and disjoint has none.
 * *first_inverted_out (may be NULL): the first pair, among those returned, whose start offset exceeds its stop
 * offset (-1: none; never with GTX_OFFSET_SKIP_REF_GAPS).
 *
 * gtx_pair_offsets_device: the entries of the pairs gtx_join_device left in HBM -- n_reads single-interval
 * queries (its n_done), d_offsets (int64[n_reads + 1], from 0), d_pairs (int32[n_pairs]) -- into d_out
 * (int64[2 * n_pairs]), op as above, the reference region the point.  Returns with the work complete. */
#define GTX_OFFSET_1        1    /* -op 1: the start of the front interval                                     */
#define GTX_OFFSET_2        2    /* -op 2: the stop of the back interval                                       */
#define GTX_OFFSET_5P       3    /* -op 5p: + the start of the front interval, - the stop of the back one      */
#define GTX_OFFSET_3P       4    /* -op 3p: + the stop of the back interval, - the start of the front one      */
#define GTX_OFFSET_SKIP_REF_GAPS 64u   /* gtx_join_offsets: --skip-ref-gaps                                     */
#define GTX_OFFSET_FROM_QUERY   128u   /* gtx_join_offsets: the query is the reference point (offset -S)        */
int gtx_set_ref_strands(gtx_ctx *ctx, const int8_t *strand /* n_refs of '+' / '-', or NULL = '+' */);
int gtx_join_offsets(gtx_ctx *ctx, const int32_t *read_triples, const int64_t *first /* n + 1, or NULL */, const int32_t *blocks,
                     const int8_t *read_strands /* n_reads, or NULL */, int64_t n_reads, uint32_t flags, int32_t op,
                     int64_t *offsets_out /* n_reads + 1 */, int32_t *pairs_out, int64_t pair_capacity,
                     int64_t *entry_offsets_out /* pair_capacity + 1 */, int64_t *entries_out /* 2 x entry_capacity */,
                     int64_t entry_capacity, int64_t *first_inverted_out /* may be NULL */, gtx_count_info *info /* may be NULL */);
int gtx_pair_offsets_device(gtx_ctx *ctx, const void *d_read_triples, int64_t n_reads, const void *d_offsets, const void *d_pairs,
                            int64_t n_pairs, int32_t op, void *d_out /* int64[2 * n_pairs] */,
                            int64_t *first_inverted_out /* may be NULL */);

/* ---- genomic_overlaps annotate: gene and upstream hits kept on the device ---------------------- */

/* genomic_overlaps annotate (gtools/genomic_overlaps.cpp:310-353) reports, for every test region, the genes it
 * overlaps and then the upstream regions it overlaps (CreateGenomicRegionSetAnnotator,
 * genomic_intervals.cpp:6218-6297), each pair through PrintAnnotations (:268-290): the 5' offsets of the test
 * region for a gene, the 3' offsets for an upstream region, and under --query-op center only the pairs whose
 * centre offset (start + stop offset) / 2 is not negative.  Genes and upstream regions are ONE reference set
 * here: ordinals below n_primary are the genes, the others the upstream regions, and an order key
 * (gtx_set_ref_order) that ranks every gene before every upstream region makes one join hand out a query's
 * pairs in the order the reference prints them.  Strands come from gtx_set_ref_strands.
 *
 * gtx_pair_annotate_device: over the pairs gtx_join_device left in HBM (d_read_triples, n_reads, d_offsets,
 * d_pairs, n_pairs as for gtx_pair_offsets_device) the offsets with op_primary for ordinals < n_primary and
 * op_rest for the rest (GTX_OFFSET_*).  mode GTX_ANNOTATE_CENTER keeps the pairs with start + stop offset >= 0
 * and gives that sum as their value (the caller halves: the .5 stays exact); GTX_ANNOTATE_START keeps every pair
 * and gives its start offset.  d_kept_offsets (int64[n_reads + 1], from 0) are the positions of each query's
 * kept pairs, in pair order; d_kept_ref (int32) / d_kept_value (int64) receive the first `capacity` kept pairs;
 * *n_kept_out is the number kept whatever the capacity: when it exceeds the capacity, grow and call again.
 * Returns with the work complete.
 *
 * gtx_join_annotate: single-interval queries from host memory, joined in gtx_join's batches and chunks (a query
 * with more pairs than the join buffer alone in a buffer of its size), each chunk's pairs annotated where they
 * lie; the host receives the kept CSR alone -- kept_offsets_out (n_reads + 1) always complete, the first
 * `capacity` kept pairs, *n_pairs_out = the pairs of the join.  flags, info: as gtx_join. */
#define GTX_ANNOTATE_CENTER 1    /* --query-op center  */
#define GTX_ANNOTATE_START  2    /* --query-op overlap */
int gtx_pair_annotate_device(gtx_ctx *ctx, const void *d_read_triples, int64_t n_reads, const void *d_offsets, const void *d_pairs,
                             int64_t n_pairs, int64_t n_primary, int32_t op_primary, int32_t op_rest, int32_t mode,
                             void *d_kept_offsets /* int64[n_reads + 1] */, void *d_kept_ref /* int32[capacity] */,
                             void *d_kept_value /* int64[capacity] */, int64_t capacity, int64_t *n_kept_out /* may be NULL */);
int gtx_join_annotate(gtx_ctx *ctx, const int32_t *read_triples, int64_t n_reads, uint32_t flags, int64_t n_primary,
                      int32_t op_primary, int32_t op_rest, int32_t mode, int64_t *kept_offsets_out /* n_reads + 1 */,
                      int32_t *kept_ref_out, int64_t *kept_value_out, int64_t capacity, int64_t *n_pairs_out /* may be NULL */,
                      gtx_count_info *info /* may be NULL */);

/* ---- genomic_apps profile / heatmap: signal binned around reference points ---------------------- */

/* genomic_apps profile and heatmap (gtools/genomic_apps.cpp:560-605, :826-880) sum, for every (read, reference
 * region) pair of the bin index, the read's weight into the bin of its offset from the region's 5' point: the
 * start / stop offset {a, b} of the read's FRONT interval (GetOffsetFrom, genomic_intervals.cpp:646-667, op 5p),
 *     x = (double)(a + b) / 2 / ref_len + bin_min,  z = (x - bin_min) / (bin_max - bin_min),
 * and, when 0 <= z < 1, bins[(int)(n_bins * z)] += w -- each step in double, in that order, without fused
 * multiply-adds.  The pairs are those of gtx_join with the same flags; the regions are the set of gtx_set_refs[_ex]
 * with its gtx_set_ref_blocks intervals and gtx_set_ref_strands strands (the caller shifts them as the reference does
 * before it builds its index).  The pairs are not materialised: one pass walks, offsets, bins and accumulates.
 *
 * gtx_set_signal_bins: the bin geometry, and ref_len (n_refs values, a size_t each; NULL = 1) for --norm-ref-length.
 * n_bins in [0, 2^31).  gtx_set_refs clears it.
 *
 * Weights are int64 (NULL: 1 per read) and the bins int64 sums (wrap-around).  While every weight is an integer and
 * no partial sum reaches 2^53 in magnitude, (double)bins[k] is bit-equal to the reference's sequential double sum;
 * info->weight_abs_sum bounds every partial sum.  A pair with (int)(n_bins * z) == n_bins is dropped and counted in
 * n_dropped (the reference would write past its array there).  With IEEE doubles that cannot happen: for an integer
 * n_bins < 2^53 and z <= 1 - 2^-53, n_bins * z rounds below n_bins (tests/test_switch_points_cpu.py), so the guard is
 * free and n_dropped stays 0.
 * *first_inverted_out (may be NULL): the first read with a pair whose start offset exceeds its stop offset (the
 * reference's "this must be a bug" exit; such pairs are not binned), -1: none.
 *
 * Layout: one row of n_bins (profile), or with GTX_SIGNAL_PER_REF one row per reference ordinal (heatmap,
 * n_refs x n_bins, row-major).
 *
 * gtx_signal_bins: reads from host memory (triples; multi-interval reads as in gtx_join: first / blocks, NULL when
 * every read has one interval), in batches; bins_out (the layout above) is ADDED to.  gtx_signal_bins_device:
 * single-interval triples and weights (int64, may be NULL) in HBM; d_bins (int64, the layout above) is added to.
 * Both return with the work complete.  flags: GTX_ZERO_LENGTH_OK, GTX_JOIN_GAPS, GTX_SIGNAL_PER_REF. */
#define GTX_SIGNAL_PER_REF 256u   /* gtx_signal_bins*: one row of bins per reference region (heatmap)          */
typedef struct gtx_signal_info {
  int64_t n_pairs;          /* pairs walked                                                           */
  int64_t n_binned;         /* pairs that landed in a bin                                             */
  int64_t n_dropped;        /* pairs with 0 <= z < 1 but bin == n_bins                                */
  int64_t weight_abs_sum;   /* sum of |w| over the binned pairs                                       */
  int64_t n_no_class;       /* reads whose class is outside [0, n_classes)                            */
  int64_t n_degenerate;     /* reads with start > stop (+1 under GTX_ZERO_LENGTH_OK): no pairs         */
} gtx_signal_info;
int gtx_set_signal_bins(gtx_ctx *ctx, double bin_min, double bin_max, int64_t n_bins, const int64_t *ref_len /* n_refs, or NULL = 1 */);
int gtx_signal_bins(gtx_ctx *ctx, const int32_t *read_triples, const int64_t *first /* n + 1, or NULL */, const int32_t *blocks,
                    const int64_t *weights /* n_reads, or NULL = 1 */, int64_t n_reads, uint32_t flags, int64_t *bins_out,
                    int64_t *first_inverted_out /* may be NULL */, gtx_signal_info *info /* may be NULL */);
int gtx_signal_bins_device(gtx_ctx *ctx, const void *d_read_triples, const void *d_weights /* int64, may be NULL */, int64_t n_reads,
                           uint32_t flags, void *d_bins, int64_t *first_inverted_out /* may be NULL */,
                           gtx_signal_info *info /* may be NULL */);

/* ---- genomic_overlaps coverage / density ------------------------------------------------- */

/* Replaces GenomicRegionSetOverlaps::CalcIndexCoverage (genomic_intervals.cpp:5269-5285, decl
 * genomic_intervals.h:2455) for single-interval regions:
 *     cov[k] = sum over reads q overlapping reference k of w_q * (min(e_q,E_k) - max(s_q,S_k) + 1)
 * in FILE order, 64-bit wrap-around arithmetic.  Same calling pattern as the count entry points; the
 * reference set is the one given to gtx_set_refs[_ex].  Reads and regions of zero length contribute 0
 * (both CalcOverlap and the -gaps formula yield 0 for them). */
int gtx_coverage_begin(gtx_ctx *ctx);
int gtx_coverage_add(gtx_ctx *ctx, const int32_t *read_triples, const int32_t *weights, int64_t n_reads, uint32_t flags);
int gtx_coverage_end(gtx_ctx *ctx, uint64_t *cov_out /* n_refs */, gtx_count_info *info /* may be NULL */);
int gtx_coverage(gtx_ctx *ctx, const int32_t *read_triples, const int32_t *weights, int64_t n_reads,
                 uint32_t flags, uint64_t *cov_out /* n_refs */, gtx_count_info *info /* may be NULL */);
int gtx_coverage_device(gtx_ctx *ctx, const void *d_read_triples, const void *d_weights, int64_t n_reads,
                        uint32_t flags, void *d_cov_out);

/* ---- genomic_scans counts --------------------------------------------------------------- */

/* Number of sliding windows the scanners report for a chromosome of length `len`
 * (genomic_intervals.cpp:5025, :5061-5064): n = len/win_step micro-windows, c = win_size/win_step,
 * max(0, n - c + 1) windows; window k (0-based) is [win_step*k + 1, win_step*k + win_size] (:5111). */
int64_t gtx_scan_n_windows(int64_t len, int64_t win_step, int64_t win_size);

/* Replaces the UnsortedGenomicRegionSetScanner constructor (genomic_intervals.cpp:5019-5080)
 * -- equivalently the window sums SortedGenomicRegionSetScanner::Next (:4928-4957) yields:
 * per class c, micro-window histogram v[(pos-1)/win_step] += w_q for reads with start <= end,
 * end > 0, pos >= 1 inside the first class_len[c]/win_step micro-windows
 * (pos = start for preprocess '1', start + (end-start)/2 for 'c'), then sums of
 * win_size/win_step consecutive micro-windows.  windows_out is the concatenation over classes,
 * class c at class_offsets[c], gtx_scan_n_windows(class_len[c],..) entries each. */
int gtx_scan(gtx_ctx *ctx, const int32_t *read_triples, const int32_t *weights, int64_t n_reads,
             const int32_t *class_len, int32_t n_classes, int32_t win_step, int32_t win_size, char preprocess,
             uint32_t flags, uint64_t *windows_out, const int64_t *class_offsets);

/* Device-resident form: d_windows_out uint64[total windows] in HBM; asynchronous. */
int gtx_scan_device(gtx_ctx *ctx, const void *d_read_triples, const void *d_weights, int64_t n_reads,
                    const int32_t *class_len, int32_t n_classes, int32_t win_step, int32_t win_size, char preprocess,
                    uint32_t flags, void *d_windows_out, const int64_t *class_offsets);

/* ---- several GPUs of one node ------------------------------------------------------------ */

/* Two regions overlap only inside one class (genomic_intervals.cpp:624-630), so a class is an independent unit of work.
 * A group has one member (context) per device; classes are dealt to the members (longest-processing-time packing of a
 * per-class load), every member holds the whole reference set and counts the reads of ITS classes.  What follows a member's
 * streaming kernel shrinks with its share: it finalizes only the histogram tiles of its classes and only its regions, into
 * its piece of a COMPACT vector (regions ordered by owner of their class, then position in the file: gtx_group_plan), the
 * pieces travel to member 0 over xGMI -- one grouped RCCL send / receive per member: the reduce(sum) of the per-region
 * vector with its addends known to be disjoint by class -- and member 0 puts them into file order.  genomic_scans windows
 * are per class too: a member scans its classes into a packed vector of its own, the per-class pieces travel the same way.
 * A group is ONE process and one caller thread driving all members (gtx_group_create; calls enqueue and return), or one
 * process per member (gtx_group_create_rank).  What the reference's single loop over queries
 * (genomic_intervals.cpp:5304-5317) becomes on a node. */
typedef struct gtx_group gtx_group;

/* device_ids == NULL: devices 0 .. n_devices-1.  NULL on failure (gtx_group_last_error(NULL) has the text).  librccl is
 * loaded at run time, for groups of more than one device only.  RCCL prints a version banner on stdout when a communicator
 * comes up: descriptor 1 points at stderr for the duration of that step, so a caller with other threads writing to stdout
 * keeps them from flushing it until gtx_group_create / gtx_group_create_rank has returned. */
gtx_group  *gtx_group_create(int n_devices, const int *device_ids);
/* One process per member: rank 0 obtains an id (GTX_GROUP_ID_BYTES bytes, an ncclUniqueId) and hands it to the others by
 * whatever launched them; every process then creates its member.  The object holds the local member only; the calls that
 * take per-member arrays (gtx_group_count_device, gtx_group_scan_device) take arrays of ONE entry, results arrive on rank
 * 0, and every rank makes the same calls in the same order.  The host-buffer calls need a group that holds all its members. */
#define GTX_GROUP_ID_BYTES 128
int         gtx_group_unique_id(void *id_out /* GTX_GROUP_ID_BYTES */);
gtx_group  *gtx_group_create_rank(int device_id, int rank, int world_size, const void *unique_id /* may be NULL for a world of one */);
void        gtx_group_destroy(gtx_group *g);
int         gtx_group_size(const gtx_group *g);     /* members, all processes together */
int         gtx_group_rank(const gtx_group *g);     /* -1: the group holds all its members */
gtx_ctx    *gtx_group_ctx(gtx_group *g, int member);   /* NULL for another process's member */
const char *gtx_group_last_error(const gtx_group *g);

/* class -> member by LPT packing of class_load (e.g. reads per class, or chromosome lengths); owner_out (n_classes, may be
 * NULL) receives the assignment.  Without this call gtx_group_set_refs assigns by the span of each class's reference
 * regions and the scans by class_len.  gtx_lpt_assign is the packing itself (no group, no GPU; deterministic, so the ranks
 * of a multi-process group all compute the same). */
int  gtx_group_assign(gtx_group *g, const int64_t *class_load, int32_t n_classes, int32_t *owner_out);
void gtx_lpt_assign(const int64_t *class_load, int32_t n_classes, int n_members, int32_t *owner_out);
/* The compact order of a group's result (no group, no GPU): ref_class[k * stride] = class of region k (stride 3 reads the
 * class column of packed triples); perm[j] = file position of the region at compact position j, member m's piece =
 * positions seg_offset[m] .. seg_offset[m+1]; regions of no class (a placeholder, an id beyond the assignment) are member 0's. */
int  gtx_group_plan(const int32_t *ref_class, int64_t stride, int64_t n_refs, const int32_t *owner, int32_t n_classes, int n_members,
                    int64_t *seg_offset /* n_members + 1 */, int32_t *perm /* n_refs */);

/* gtx_set_refs_ex on every local member. */
int gtx_group_set_refs(gtx_group *g, const int32_t *ref_triples, int64_t n_refs, int32_t n_classes, uint32_t flags);

/* The reads of every member already resident in ITS device's HBM (member m: the reads of the classes it owns -- reads of
 * other classes would be counted into tiles nobody finalizes): d_reads / d_weights / n_reads are indexed by local member
 * (d_weights may be NULL).  Per member the streaming kernel and the finalize step of its share, the pieces to member 0, the
 * result in file order in d_hits (n_refs uint64 on member 0's device; ignored on other ranks).  Everything is enqueued on the
 * members' streams (gtx_set_stream of gtx_group_ctx), except that the pieces travel -- and member 0 writes d_hits -- on a
 * stream of the group's own behind each member's finalize step, into one of two compact vectors in turn: the kernels of the
 * next call run under the exchange of this one.  d_hits is complete after gtx_group_sync, or, for work enqueued afterwards on
 * the members' streams, behind gtx_group_wait_result (a device-side wait, the host does not block); until then the caller
 * leaves d_hits alone (alternate two vectors to keep calls in flight).  GTX_CHECK_SORTED is ignored, GTX_ZERO_LENGTH_OK
 * refused (the sorted merge's host-side corrections live in the host-buffer calls).
 * gtx_group_last_info: the sums over the local members (first_unsorted / first_degenerate are not tracked: -1). */
int gtx_group_count_device(gtx_group *g, const void *const *d_reads, const void *const *d_weights, const int64_t *n_reads,
                           uint32_t flags, void *d_hits);
int gtx_group_scan_device(gtx_group *g, const void *const *d_reads, const void *const *d_weights, const int64_t *n_reads,
                          const int32_t *class_len, int32_t n_classes, int32_t win_step, int32_t win_size, char preprocess,
                          uint32_t flags, void *d_windows /* member 0's device, layout class_offsets */, const int64_t *class_offsets);
int gtx_group_sync(gtx_group *g);
int gtx_group_wait_result(gtx_group *g);
int gtx_group_last_info(gtx_group *g, gtx_count_info *info);

/* The streaming count / coverage calls of a single context, on the group: every read goes to the owner of its class (reads
 * of no known class to member 0).  Sorted input is cut into a few contiguous runs per batch; interleaved input is
 * partitioned on the host.  Page-locked batches (gtx_host_alloc) follow the single-context rule: a batch must stay
 * untouched until the group's next host-buffer call has returned (the call waits for every member's copy of the previous
 * batch, also of members that get nothing of the new one).  count on a plain reference set ends with the pieces of the
 * compact vector as above; coverage, and count on a GTX_REFS_KEEP_ZERO_LENGTH set (whose inverted intervals are matched
 * into the full vector), with one ncclReduce(sum) of the members' full vectors.  info: the sums over the members;
 * first_unsorted / first_degenerate are not tracked (-1), and GTX_CHECK_SORTED is ignored. */
int gtx_group_count_begin(gtx_group *g);
int gtx_group_count_add(gtx_group *g, const int32_t *read_triples, const int32_t *weights, int64_t n_reads, uint32_t flags);
int gtx_group_count_end(gtx_group *g, uint64_t *hits_out /* n_refs */, gtx_count_info *info /* may be NULL */);
/* gtx_set_ref_blocks on every member / gtx_count_add_regions on the members in turn (every member holds the whole reference set) */
int gtx_group_set_ref_blocks(gtx_group *g, const int64_t *first /* n_refs + 1, or NULL */, const int32_t *blocks);
int gtx_group_count_add_regions(gtx_group *g, const int32_t *env_triples, const int32_t *weights /* may be NULL */,
                                const int64_t *first /* n + 1 */, const int32_t *blocks, int64_t n);
int gtx_group_coverage_begin(gtx_group *g);
int gtx_group_coverage_add(gtx_group *g, const int32_t *read_triples, const int32_t *weights, int64_t n_reads, uint32_t flags);
int gtx_group_coverage_end(gtx_group *g, uint64_t *cov_out /* n_refs */, gtx_count_info *info /* may be NULL */);
/* gtx_scan on the group (arguments as gtx_scan; with more than one member only the classes' own ranges of windows_out are
 * written, whatever class_offsets leaves between them is not touched). */
int gtx_group_scan(gtx_group *g, const int32_t *read_triples, const int32_t *weights, int64_t n_reads,
                   const int32_t *class_len, int32_t n_classes, int32_t win_step, int32_t win_size, char preprocess,
                   uint32_t flags, uint64_t *windows_out, const int64_t *class_offsets);
/* reads each member received in the last (or open) group call: the load balance actually achieved */
int gtx_group_member_reads(const gtx_group *g, int64_t *reads_out /* gtx_group_size */);

/* ---- region text tokenised on the device ---------------------------------------------------
 * Ingest (GenomicRegionBED::Read genomic_intervals.cpp:2157-2182, tokenizer core.cpp:577-625, FileBufferText::Next
 * core.cpp:241-259) for the query stream of the two reductions: a block of COMPLETE lines of a BED file ('\n' after every line,
 * n_lines of them) is copied to the device as text and cut into packed triples there, then counted like a gtx_count_add /
 * gtx_coverage_add batch of an open call.  The device recognises only the plain case -- tab-separated, decimal columns 2 and 3,
 * strand column one of + - . 1 -1, not 12 columns, in the order the sorted merge requires, reads the mode accepts; the reference's
 * reading of everything else (blanks as separators, signs, '\r', BED12, its error messages with their line numbers) stays with
 * the host-side packer: a block with ANY other line is not counted at all and gtx_text_result says so -- the caller packs that
 * block itself and adds it with gtx_count_add.  chrom_names: the chromosome of class c (classes beyond n_chrom are the '-' strand
 * when strand_aware); a line of another chromosome is dropped, as the reference's index lookup does (:5719-5720).
 * sorted_rules: the sorted merge's rules (order check against the line before -- prev_* describe the line before the block --, no
 * validation of the interval), else the bin index's (stop <= 0 or start > stop is the reference's error: not plain).
 * max_label_value > 1: weights = min(max, atol(column 4)) (genomic_intervals.cpp:1081-1085). */
typedef struct gtx_text_rules {
  const char *const *chrom_names; int32_t n_chrom;
  int32_t strand_aware, sorted_rules, sorted_by_strand;
  int64_t max_label_value;
  int32_t have_prev; const char *prev_chrom; int32_t prev_strand /* '+' | '-' */; int64_t prev_start;
} gtx_text_rules;
/* GTX_TEXT_SAM in the flags of gtx_count_add_text, gtx_coverage_add_text, gtx_scan_add_text and gtx_group_*_add_text: the block is
 * SAM alignments (GenomicRegionSAM::Read genomic_intervals.cpp:2771-2812) without the '@' header, not BED.  The plain case: 11 or more
 * TAB-separated columns, the first ten non-empty and without blanks, '\r' or NUL, QUAL non-empty and not beginning with a blank, '\r'
 * or NUL (a NUL there ends the C string behind 10 tokens: the reference's error), no '\r' at the end of the line; FLAG and POS 1-10
 * decimal digits; CIGAR "*" or operations of 1-9 digits from M I D S H P X - (no N, no =); SEQ "*" or as long as the CIGAR's M I S X;
 * a reference length (M D X) > 0; with max_label_value > 1, a QNAME that begins with a byte above ' ' and has at most 18 digits.
 * A read becomes (class of RNAME [+ n_chrom when strand_aware and FLAG & 0x10], POS, POS + reference length - 1) with QNAME's atol
 * value as its label; order check and validity rules as for BED.  Spliced reads, '=' and every other line go back to the caller
 * (needs_host), as do blocks whose 128-line groups average more than ~570 bytes a line.  gtx_text_rules is the same. */
#define GTX_TEXT_SAM       512u
/* GTX_TEXT_GFF in the same flags (not together with GTX_TEXT_SAM: GTX_E_ARG): the block is GFF / GTF features (GenomicRegionGFF::Read
 * genomic_intervals.cpp:3501-3517) without the leading '##' lines, not BED.  The plain case: 8, 9 or 10 TAB-separated columns, the
 * first eight non-empty and without blanks, '\r' or NUL; columns 4 and 5 of 1-10 decimal digits without a sign, both below 2^31 - 2;
 * column 7 exactly one byte, '+' or '-'; column 9, when present, non-empty and not beginning with a byte <= ' '; column 10, when
 * present, non-empty; no '\r' at the end of the line.  A feature becomes (class of column 1 [+ n_chrom when strand_aware and column 7
 * is '-'], column 4, column 5) as written -- 1-based, inclusive -- with column 9's atol value as its label (0 for an 8-column line;
 * more than 18 digits are not plain); order check and validity rules as for BED.  A '.' or any other strand byte, a '#' comment, an
 * 11th column and every other line go back to the caller (needs_host), as do blocks whose 128-line groups average more than ~570
 * bytes a line.  gtx_text_rules is the same. */
#define GTX_TEXT_GFF      2048u
/* text: host memory (page-locked memory is read by the DMA engine directly and must stay untouched until gtx_text_result of the
 * ticket has returned).  flags as gtx_count_add / gtx_coverage_add, and GTX_TEXT_SAM or GTX_TEXT_GFF.  Up to two blocks are in flight: the call waits for the block
 * before last. */
int gtx_count_add_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket);
int gtx_coverage_add_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket);
/* waits for the tokenizer of that block; *needs_host != 0: nothing of the block was counted, the caller packs and adds it */
int gtx_text_result(gtx_ctx *ctx, int ticket, int *needs_host);
/* genomic_overlaps subset on text (gtools/genomic_overlaps.cpp:782-800): a block of complete BED lines goes to the device as for
 * gtx_count_add_text (same buffers contract, same rules, same seam key, two blocks in flight; no count call need be open), is cut
 * into triples there, gets its hits per line (gtx_query_hits_device, in line order; flags: GTX_ZERO_LENGTH_OK, GTX_JOIN_GAPS), and
 * the lines with hits > 0 -- hits == 0 under GTX_SUBSET_INVERT, the reference's -inv -- are gathered, newline included, in order.
 * The reference prints a selected region with GenomicRegionBED::Print (genomic_intervals.cpp:2188-2218), which renders the line
 * again from its parsed fields; a line is copied only where that rendering is the line itself: on top of the tokenizer's plain
 * case, 3 to 6 tab-separated tokens without blanks, '\r' or control bytes, columns 2 and 3 in canonical decimal ("0" or no leading
 * zero), column 5 a canonical long (optional '-', no leading zero, not "-0", at most 18 digits), column 6 exactly "+" or "-".
 * A block with ANY other line yields nothing: gtx_subset_result says needs_host, and the caller does that block by its own means.
 * gtx_subset_result waits for the block of that ticket; out receives the selected text (room for the block's bytes),
 * *out_bytes its length, *n_selected (may be NULL) the number of lines.  The result of a ticket must be fetched before the block
 * after next is added. */
#define GTX_SUBSET_INVERT 1024u   /* gtx_subset_text: keep the lines with hits == 0 */
int gtx_subset_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket);
int gtx_subset_result(gtx_ctx *ctx, int ticket, int *needs_host, char *out /* >= bytes of the block */, size_t *out_bytes,
                      int64_t *n_selected /* may be NULL */);
/* genomic_regions shift | shiftp | pos | center | fix | bounds on text (gtools/genomic_regions.cpp:726-727, :721, :704, :708, :703;
 * GenomicRegionSet::RunShiftPos, RunModifyPos, RunCenter, RunFix, RunBounds genomic_intervals.cpp:3954-4140): a block of complete BED
 * lines goes to the device as for gtx_subset_text (same buffers contract, two blocks in flight, tickets in order; no reference set
 * and no count call need be open) and every line is printed again with columns 2 and 3 rewritten, or dropped.  With s = column 2 + 1,
 * e = column 3 (:2163-2164), the strand '+' unless column 6 is "-" (:2165), in signed 64-bit arithmetic whose division truncates:
 *   GTX_REWRITE_SHIFT    s' = s + a, e' = e + b                                   (:524-531 with strand_aware = false)
 *   GTX_REWRITE_SHIFTP   on '-': s' = s - b, e' = e - a; else as SHIFT              (a = the 5' shift, b = the 3' shift)
 *   GTX_REWRITE_POS      pos_op C: m = s + (e - s + 1) / 2, s' = m - a, e' = m + a; else with choose_start = pos_op 1, or 5P on '+',
 *                        or 3P on '-': e' = s + a when it holds, s' = e - a when not  (:537-550; a = the -c shift)
 *   GTX_REWRITE_CENTER   s' = s + (e - s) / 2, e' = e - (e - s) / 2                 (:1293-1301)
 *   GTX_REWRITE_FIX      the line as it is when s >= 1 and s <= e, else dropped     (:333-338, :1419-1425)
 *   GTX_REWRITE_BOUNDS   dropped when column 1 is none of chrom_names (:3959) or s > L, e < 1 or e < s with L = chrom_len of that name
 *                        (:560-563, then Fix); else s' = max(s, 1), e' = min(e, L), dropped when that leaves s' > e' (:564-568, Fix)
 * A printed line is column 1, TAB, s' - 1, TAB, e' -- both "%ld", so s' - 1 may be 0 or negative -- and then the input's own bytes
 * from behind column 3 to the newline (GenomicRegionBED::Print :2188-2218): a 4-column line keeps its label, a 5-column line keeps
 * its score, a 6-column line its strand, and a 3-column line prints no label (the "_" the reader gives it is never printed, :2192).
 * That copy is Print's rendering only of a line gtx_subset_text would copy (the same predicate: the tokenizer's plain case, 3 to 6
 * tab-separated tokens without blanks, '\r' or control bytes, columns 2 and 3 canonical decimals of at most 10 digits below
 * 2^31 - 2, column 5 a canonical long, column 6 exactly "+" or "-"); a block with ANY other line, or with a tile of consecutive lines
 * (gtx_rewrite_limits) whose text or whose output is longer than the stage, yields nothing: gtx_rewrite_result says
 * needs_host with *out_bytes = 0 and the caller renders that block by its own means.  GTX_E_ARG: an amount beyond +-2^62 (the
 * caller's own loop takes those), a kind or pos_op that is none of the above.
 * gtx_rewrite_result waits for the block of that ticket; out (capacity bytes of it, gtx_rewrite_max_bytes(bytes, n_lines) of the
 * block always suffice: a line grows by at most the two rendered numbers) receives exactly *out_bytes bytes, the printed lines in
 * order; *n_printed (may be NULL) their number.  A result larger than capacity is GTX_E_ARG and nothing is written.  The result of a
 * ticket must be fetched before the block after next is added.
 * gtx_rewrite_limits: the lines per tile of the passes and the bytes of a tile's text, and of its output, that the stage holds.
 * Under gtx_profile_enable a gtx_rewrite_text call is bracketed too: ms_stream_kernel is the plan, prefix and emit launches alone, on
 * text that is already in HBM behind its newline index and tokenizer; ms_total adds the copies of the verdict and the totals. */
#define GTX_REWRITE_SHIFT  0
#define GTX_REWRITE_SHIFTP 1
#define GTX_REWRITE_POS    2
#define GTX_REWRITE_CENTER 3
#define GTX_REWRITE_FIX    4
#define GTX_REWRITE_BOUNDS 5
#define GTX_REWRITE_POS_1  0
#define GTX_REWRITE_POS_2  1
#define GTX_REWRITE_POS_5P 2
#define GTX_REWRITE_POS_3P 3
#define GTX_REWRITE_POS_C  4
typedef struct gtx_rewrite_op {
  int32_t kind, pos_op;                        /* GTX_REWRITE_*, GTX_REWRITE_POS_* (read under GTX_REWRITE_POS only) */
  int64_t a, b;                                /* the two amounts (see above); unused ones are ignored but must be in range */
  const char *const *chrom_names; const int64_t *chrom_len; int32_t n_chrom;   /* GTX_REWRITE_BOUNDS: the genome's names and lengths */
} gtx_rewrite_op;
int gtx_rewrite_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_rewrite_op *op, int *ticket);
int gtx_rewrite_result(gtx_ctx *ctx, int ticket, int *needs_host, char *out, size_t capacity, size_t *out_bytes, int64_t *n_printed /* may be NULL */);
size_t gtx_rewrite_max_bytes(size_t bytes, int64_t n_lines);
int gtx_rewrite_limits(int32_t *tile, int32_t *stage);
/* genomic_regions bed | reg on text (gtools/genomic_regions.cpp:710, :722; GenomicRegionSet::RunConvertToBED genomic_intervals.cpp
 * :3940-3948, RunConvertToREG :4097-4103): a block of complete lines of BED (flags 0), SAM (GTX_TEXT_SAM) or GFF / GTF (GTX_TEXT_GFF)
 * text without header lines goes to the device as for gtx_rewrite_text (same buffers contract, two blocks in flight, tickets in
 * order) and every line is printed as a line of another format.  CHROM, START, STOP, STRAND and LABEL of a line are what the
 * reference's readers give (:2771-2812 and :2870-2873, :3501-3517, :2157-2172): SAM -- RNAME, POS, POS + the CIGAR's reference length
 * - 1 (as GTX_TEXT_SAM above states it; "*" counts as len(SEQ) M), '-' when FLAG & 0x10, QNAME; GFF -- columns 1, 4, 5, 7 and 9, "_"
 * on an 8-column line; BED -- column 1, column 2 + 1, column 3, '-' when column 6 is "-", column 4 or "_" on a 3-column line.
 *   GTX_CONVERT_BED   CHROM' TAB START-1 TAB STOP TAB LABEL TAB 1000 TAB STRAND [TAB START-1 TAB STOP TAB color] NL   (:1256-1274)
 *                     the bracket when color is not empty; CHROM' is CHROM, under ucsc_names "chr" + CHROM with "MT" printed as
 *                     "chrM" (:5968-5972); numbers are "%ld", so START-1 is -1 for a read with POS 0.  SAM and GFF text only: BED
 *                     text is GTX_E_ARG (the reference prints a BED line through its own class, which is not converted here)
 *   GTX_CONVERT_REG   LABEL TAB CHROM SP STRAND SP START SP STOP NL   (:961-971 over :843-849 and :344-347; the compact form of a
 *                     single-interval region is the same bytes); ucsc_names and color are not read
 * The track and browser lines in front of the first region (:3944-3945) are the caller's to print.  The lines the device takes are
 * the tokenizer's plain case of the format, and for BED text those of gtx_rewrite_text; a block with ANY other line -- a spliced read,
 * a '=' operation, a '.' strand, BED12 -- or with a tile of consecutive lines (gtx_convert_limits) whose output is longer than the
 * stage, yields nothing: gtx_convert_result says needs_host with *out_bytes = 0 and the caller renders that block by its own means.
 * GTX_E_ARG: both format flags, a flag that is neither, a `to` that is neither of the two, BED text with GTX_CONVERT_BED, a color
 * longer than max_color of gtx_convert_limits.
 * gtx_convert_result waits for the block of that ticket; out (capacity bytes of it) receives exactly *out_bytes bytes, the printed
 * lines in order; *n_printed (may be NULL) their number, which is the block's.  A result larger than capacity is GTX_E_ARG and
 * nothing is written.  The result of a ticket must be fetched before the block after next is added.
 * gtx_convert_max_bytes(bytes, n_lines, op) always suffices.  A printed line holds its input line's chromosome and label, which are
 * c and l bytes of that line, and beside them at most: bed -- 3 ("chr") + 1 + 10 + 1 + 10 + 1 + 6 ("\t1000\t") + 1 (strand) + 1
 * (newline) = 34 bytes, one more where the label is the "_" the input does not hold (coordinates are below 2^31 - 2, so a number has
 * at most 10 bytes, "-1" included), and with a color 1 + 10 + 1 + 10 + 1 = 23 and the color's bytes on top; reg -- 1 + 1 + 1 + 1 + 10
 * + 1 + 10 + 1 = 26, one more for "_".  So the bound is bytes + n_lines * (35 [+ 23 + strlen(color)]).
 * gtx_convert_limits: the lines per tile of the passes, the bytes of a tile's output that the stage holds, the longest color.
 * Under gtx_profile_enable a gtx_convert_text call is bracketed as gtx_rewrite_text is (ms_stream_kernel: plan, prefix and emit). */
#define GTX_CONVERT_BED 0
#define GTX_CONVERT_REG 1
typedef struct gtx_convert_op {
  int32_t to;                                  /* GTX_CONVERT_BED | GTX_CONVERT_REG */
  int32_t ucsc_names;                          /* -chr */
  const char *color;                           /* NULL or "": none; at most gtx_convert_limits' max_color bytes, else GTX_E_ARG */
} gtx_convert_op;
int gtx_convert_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_convert_op *op, uint32_t flags, int *ticket);
int gtx_convert_result(gtx_ctx *ctx, int ticket, int *needs_host, char *out, size_t capacity, size_t *out_bytes, int64_t *n_printed /* may be NULL */);
size_t gtx_convert_max_bytes(size_t bytes, int64_t n_lines, const gtx_convert_op *op);
int gtx_convert_limits(int32_t *tile, int32_t *stage, int32_t *max_color);
/* The same in a group that holds all its members (between gtx_group_count_begin / gtx_group_coverage_begin and their _end): a block goes
 * to the members in turn, whatever the classes of its lines -- the read stream split evenly over members that each hold the whole
 * reference set (SURVEY 8(e)'s second partition) -- and a count call that took text blocks ends with the ncclReduce(sum) of the
 * members' full vectors instead of pieces.  Blocks that come back (needs_host) are packed by the caller and go through gtx_group_*_add. */
int gtx_group_count_add_text(gtx_group *g, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket);
int gtx_group_coverage_add_text(gtx_group *g, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket);
int gtx_group_text_result(gtx_group *g, int ticket, int *needs_host);

/* Regions into position order on the device: what the reference's bin/sortbed (`sort -k1,1 -k2,2n`, or
 * `-k1,1 -k6,6 -k2,2n`) and `genomic_regions gsort` (RunGlobalSort genomic_intervals.cpp:4547-4570 over BinGenomicRegions :6095-6150
 * and CompareBinnedGenomicRegions :6044-6048) are run for -- the input order the sorted merge (:5807-5937) and the sorted scanner
 * (:4928-4957) insist on.  order[i] = the input ordinal of the region that comes i-th under (class ascending, start ascending, stop
 * DESCENDING, input order): gsort's order when the caller folds the chromosome's strcmp rank -- and, sorting by strand, the strand
 * below it -- into the class.  sorted (may be NULL) receives the triples in that order.  n_reads < 2^32; a class id outside
 * [0, n_classes) is GTX_E_RANGE.  No reference set is needed.  gtx_sort_device: reads, order (uint32[n_reads]) and sorted in the
 * context's HBM; the call returns when the result is complete. */
int gtx_sort(gtx_ctx *ctx, const int32_t *read_triples, int64_t n_reads, int32_t n_classes, uint32_t *order_out, int32_t *sorted_out);
int gtx_sort_device(gtx_ctx *ctx, const void *d_reads, int64_t n_reads, int32_t n_classes, void *d_order, void *d_sorted);

/* A position-sorted region stream merged into its covered territory: the reference's `genomic_regions link [-s] [-d N] [--label-func F]`
 * (genomic_regions.cpp:437-451, 546-550, 704, 744; RunGlobalLink genomic_intervals.cpp:4605-4644 over Next :3874-3882, IsBefore :396-401,
 * IsCompatibleWith :416-421, PrintModified :909-913) -- what `bedtools merge` does.  The loop: the first region is the head of a group
 * and new_stop its STOP; a following region joins while it is compatible with the head (same class: the caller folds the chromosome
 * and, under -s, the strand into the class id, as everywhere in this header; ANY int32 is a class, there is no n_classes and no
 * reference set) and START - new_stop <= max_difference, and then new_stop = max(STOP, new_stop); otherwise the group is closed and the
 * region heads the next one.  max_difference may be negative; 0 joins overlapping regions but not adjacent ones (coordinates are the
 * set's: BED start + 1, stop).
 * The parallel form the kernels compute: within a class the starts do not decrease (anything else is the order error below), so region
 * i heads a group exactly when it is the first of its class or START[i] - P[i-1] > max_difference, P[i-1] the largest STOP of ALL
 * regions of the class in front of it (a group closed earlier at j had START[j] - its maximum > d and START[i] >= START[j]: its
 * maximum never decides for i).  The difference is taken in 64 bits.  A group's new_stop is the maximum over ITS members, which P is
 * not when max_difference < 0 or an interval is inverted.
 * Per group g, in stream order: head[g] = the ordinal of its first region, count[g] = its members, stop[g] = new_stop, and with one of
 * the fold flags value[g] = the sum (two's complement) / minimum / maximum of the members' int64 values.  info->n_groups = the groups
 * written.  info->first_unsorted = the first region that is before its predecessor in (class, start) -- Next's "input regions are not
 * sorted" -- or -1; groups are reported only for the prefix in front of it, and the group open at that region is not among them (the
 * reference prints the groups closed before the offending line and stops).  Outputs hold n entries.  n < 2^32 (else GTX_E_ARG); two
 * fold flags, or a fold flag without values / value_out, are GTX_E_ARG.  gtx_link_device: all pointers but info in the context's HBM,
 * enqueued on its stream; *info is valid after gtx_sync (and must live until then). */
#define GTX_LINK_SUM 1u   /* fold the values: at most one of the three */
#define GTX_LINK_MIN 2u
#define GTX_LINK_MAX 4u
#define GTX_LINK_TILE 2048   /* regions per block of the scans (what tests place their boundary cases by) */
typedef struct gtx_link_info { int64_t n_groups, first_unsorted; } gtx_link_info;
int gtx_link(gtx_ctx *ctx, const int32_t *triples, const int64_t *values /* may be NULL */, int64_t n, int64_t max_difference,
             uint32_t flags, uint32_t *head_out, uint32_t *count_out, int32_t *stop_out, int64_t *value_out /* may be NULL */,
             gtx_link_info *info);
int gtx_link_device(gtx_ctx *ctx, const void *d_triples, const void *d_values, int64_t n, int64_t max_difference, uint32_t flags,
                    void *d_head, void *d_count, void *d_stop, void *d_value, gtx_link_info *info);

/* Link fed block by block (the path of `genomic_regions link` for BED text): gtx_link_text_begin opens a call for at most `capacity`
 * regions over n_chrom chromosome names (the caller's table, ids in strcmp order; sorted_by_strand: the strand is folded below the id
 * into link's class).  gtx_link_add_text tokenises a block of complete lines on the device (rules: the table, strand_aware = 1, no
 * order and no label rules; zero-length and inverted regions are taken) and, when every line of it is plain, appends its regions in
 * line order -- the text's triples never exist on the host; a block with anything else in it (*needs_host = 1) appends nothing and
 * is packed by the caller, who hands its regions to gtx_link_add (link classes, one strand byte -- 0 '+', 1 '-' -- per region).
 * gtx_link_text_end runs gtx_link over what was collected (no fold) and writes, per group, head, stop and the head's key
 * {2 * chromosome id + strand, START} (head_key_out: 2 int32 per group), with info as for gtx_link.  The calls synchronise. */
int gtx_link_text_begin(gtx_ctx *ctx, int32_t n_chrom, int sorted_by_strand, int64_t capacity);
int gtx_link_add_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, int *needs_host);
int gtx_link_add(gtx_ctx *ctx, const int32_t *triples, const uint8_t *minus, int64_t n);
int gtx_link_text_end(gtx_ctx *ctx, int64_t max_difference, uint32_t *head_out, int32_t *stop_out, int32_t *head_key_out, gtx_link_info *info);

/* The neighbour passes over a position-sorted region stream: the reference's `genomic_regions test [-s]`, `gdist [-op1 X] [-op2 Y]`
 * and `inv -g GENOME` (genomic_regions.cpp:413-419, 429-435, 445-451, 525-528, 536-538, 627-629, 741-745).  All three compare a
 * region with the one directly in front of it; nothing is carried along the stream.  Classes as for gtx_link: the caller folds the
 * chromosome's strcmp rank and, sorting by strand, the strand below it into the class id; for gtx_adjacent any int32 is a class.
 * n < 2^32 (else GTX_E_ARG); n = 0 is legal and writes nothing.
 *
 * gtx_adjacent (RunGlobalTest genomic_intervals.cpp:4755-4778, RunGlobalCalcDistances :4523-4542): info->first_unsorted = the first
 * region that is before its predecessor in (class, start) (IsBefore :396-401), or -1.  n_inclusions / n_overlaps, over ALL pairs
 * (i - 1, i) of one class (IsCompatibleWith :416-421) whatever first_unsorted says: with START[i] <= STOP[i - 1] the pair is an
 * inclusion when STOP[i] <= STOP[i - 1] and an overlap otherwise (:4765-4769; the predecessor, not a running maximum).  dist_out (may
 * be NULL): one int64 per region -- for i >= 1 in its predecessor's class coord(i, op2) - coord(i - 1, op1) (CalcDistanceFrom
 * :438-441), coord by GetCoordinate (:465-472): GTX_POINT_START, GTX_POINT_STOP, or the 5' / 3' end by the region's own strand
 * (minus[i] != 0: '-'; minus = NULL: all '+'); INT64_MIN for region 0 and after a class change (the reference's NaN).  An op outside
 * 0..3 is GTX_E_ARG.  gtx_adjacent_device: the pointers but info in the context's HBM, enqueued on its stream; *info is valid after
 * gtx_sync (and must live until then).
 *
 * gtx_gaps (RunGlobalInvert :4576-4600): a run is a maximal stretch of consecutive regions of one class.  bounds[c] is class c's size
 * (< 0: missing), a bound above 2^31 - 3 is GTX_E_RANGE.  The head of a run owns the gap [1, START - 1] when START > 1 (:4587); every
 * other region the gap [pSTOP + 1, START - 1] when START > pSTOP + 1, pSTOP the STOP of the region directly in front of it (:4592;
 * taken in 64 bits); the last region of a run then owns [STOP + 1, size] when STOP + 1 < size (:4596).  A region is bad when it is
 * inside a run and START < its predecessor's START (bad_kind 1: the order error, :4591) or heads a run whose class is outside
 * [0, n_bounds) or has no bound (bad_kind 2: "chromosome not found", :4585).  info->first_bad = the first bad region or -1, and exactly
 * the gaps owned by the regions in front of it are reported, in stream order: owner (the region's ordinal), start, stop.
 * info->n_gaps is their number whatever the capacity; when it exceeds capacity only the first `capacity` gaps have been written and
 * nothing behind them: grow the buffers and call again (the policy of gtx_window_select).  bounds is host memory in both entries.
 * gtx_gaps_device: triples and outputs in the context's HBM, enqueued; *info is valid after gtx_sync.
 * Tiles of GTX_ADJACENT_TILE regions; the bounds sit in LDS up to 4096 classes and are read through L2 beyond that. */
#define GTX_ADJACENT_TILE 2048   /* regions per block of the passes (what tests place their boundary cases by) */
#define GTX_POINT_START 0        /* "1"  */
#define GTX_POINT_STOP  1        /* "2"  */
#define GTX_POINT_5P    2        /* "5p" */
#define GTX_POINT_3P    3        /* "3p" */
typedef struct gtx_adjacent_info { int64_t first_unsorted /* -1: none */, n_inclusions, n_overlaps; } gtx_adjacent_info;
int gtx_adjacent(gtx_ctx *ctx, const int32_t *triples, const uint8_t *minus /* NULL: all '+' */, int64_t n, int op1, int op2,
                 int64_t *dist_out /* may be NULL */, gtx_adjacent_info *info);
int gtx_adjacent_device(gtx_ctx *ctx, const void *d_triples, const void *d_minus, int64_t n, int op1, int op2, void *d_dist,
                        gtx_adjacent_info *info);
typedef struct gtx_gaps_info { int64_t n_gaps /* needed, may exceed capacity */, first_bad /* -1: none */; int32_t bad_kind /* 0 none, 1 order, 2 no bound */; } gtx_gaps_info;
int gtx_gaps(gtx_ctx *ctx, const int32_t *triples, int64_t n, const int64_t *bounds, int32_t n_bounds, int64_t capacity,
             uint32_t *owner_out, int32_t *start_out, int32_t *stop_out, gtx_gaps_info *info);
int gtx_gaps_device(gtx_ctx *ctx, const void *d_triples, int64_t n, const int64_t *bounds, int32_t n_bounds, int64_t capacity,
                    void *d_owner, void *d_start, void *d_stop, gtx_gaps_info *info);

/* genomic_scans counts fed as a stream (UnsortedGenomicRegionSetScanner ctor genomic_intervals.cpp:5019-5080, sorted scanner :4928-4957):
 * gtx_scan_begin fixes the geometry (arguments as gtx_scan; flags: GTX_ZERO_LENGTH_OK = the sorted scanner's rule; weighted != 0: every
 * batch brings label weights), gtx_scan_add adds packed reads from host memory (flags: GTX_READS_UNSORTED as a hint), gtx_scan_add_text a
 * block of BED text tokenised on the device (rules as for the overlap calls; lines the device does not take come back through
 * gtx_text_result and are packed by the caller), gtx_scan_end writes the windows (layout of gtx_scan) and, when label_sum is not NULL,
 * the sum of the label values of all lines of the text blocks that did NOT come back (CountGenomicRegions, :6206-6214: peaks' read
 * total).  The micro-window histogram accumulates over the batches; a caller with every read in hand uses gtx_scan / gtx_scan_device. */
int gtx_scan_begin(gtx_ctx *ctx, const int32_t *class_len, int32_t n_classes, int32_t win_step, int32_t win_size, char preprocess,
                   uint32_t flags, int weighted, const int64_t *class_offsets);
int gtx_scan_add(gtx_ctx *ctx, const int32_t *read_triples, const int32_t *weights, int64_t n_reads, uint32_t flags);
int gtx_scan_add_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_text_rules *rules, uint32_t flags, int *ticket);
int gtx_scan_end(gtx_ctx *ctx, uint64_t *windows_out, int64_t *label_sum);

/* Scan results that stay on the device.  gtx_scan_end_keep is gtx_scan_end with the window sums written into one of
 * GTX_SCAN_KEEP_SLOTS vectors the context owns (layout of gtx_scan, gaps between classes zero) instead of host memory; what the slot
 * held is replaced.  gtx_scan_kept gives a slot's device address and its number of windows (GTX_E_STATE for an empty slot);
 * gtx_scan_drop frees one slot, slot -1 all of them.  A slot outside [0, GTX_SCAN_KEEP_SLOTS) is GTX_E_ARG.  No other call touches
 * a kept vector. */
#define GTX_SCAN_KEEP_SLOTS 8
int gtx_scan_end_keep(gtx_ctx *ctx, int slot, int64_t *label_sum);
int gtx_scan_kept(gtx_ctx *ctx, int slot, void **d_windows, int64_t *n_windows);
int gtx_scan_drop(gtx_ctx *ctx, int slot);
/* A kept slot's window sums brought to host memory after all (layout of gtx_scan; the slot stays as it is): for the caller that
 * finds out only after the scan that it has to walk the windows itself.  An empty slot is GTX_E_STATE, a NULL buffer for a slot that
 * holds windows GTX_E_ARG. */
int gtx_scan_kept_read(gtx_ctx *ctx, int slot, uint64_t *windows_out);

/* Window selection: the data pass of `genomic_apps peakdiff` (ScanReadFiles, genomic_apps.cpp:385-412) over window vectors in HBM.
 * d_tested: n_tested (1..4) device vectors of n_windows uint64 sums; d_control: NULL (or all entries NULL), or one control vector per
 * tested vector -- a control for some only is GTX_E_ARG.  window_size is the clamp W >= 1.  kcrit[f] (host memory) is tested vector
 * f's table of critical counts: int32[W + 1] with controls, int32[1] without.  With k_f = min(v_f, W) and c_f = min(ctl_f, W), a window
 * is kept when k_f >= kcrit[f][c_f] for any f (kcrit[f][0] without controls).  The kept windows come out in window order: ordinals
 * (int64[capacity]) and rows (int32[capacity * columns], columns = n_tested, or 2 * n_tested with controls: the clamped tested counts,
 * then the clamped control counts).  *n_kept is the number of kept windows whatever the capacity; when it exceeds capacity only the
 * first `capacity` windows have been written and nothing behind them: grow the buffers and call again (the policy of gtx_join).  The
 * vectors must be 16-byte aligned (kept slots are).  gtx_window_select_device writes device buffers and returns when the result is
 * complete; gtx_window_select brings the result to host memory.  Three launches over tiles of `tile` windows (count, prefix, emit);
 * the tables sit in LDS while n_tested * (W + 1) * 4 bytes <= 64 KB and are read through L2 beyond that: gtx_window_select_limits
 * reports the tile and the largest W of the LDS path for four tested vectors with controls (n tested vectors: (lds_max_w + 1) * 4 / n - 1). */
int gtx_window_select_limits(int32_t *tile, int32_t *lds_max_w);
int gtx_window_select_device(gtx_ctx *ctx, const void *const *d_tested, const void *const *d_control, int32_t n_tested, int64_t n_windows,
                             int32_t window_size, const int32_t *const *kcrit, int64_t capacity, void *d_ordinals, void *d_rows, int64_t *n_kept);
int gtx_window_select(gtx_ctx *ctx, const void *const *d_tested, const void *const *d_control, int32_t n_tested, int64_t n_windows,
                      int32_t window_size, const int32_t *const *kcrit, int64_t capacity, int64_t *ordinals, int32_t *rows, int64_t *n_kept);

/* Window filter: the -r filter of `genomic_scans counts` over a window vector in HBM -- GenomicRegionSetIndex::GetOverlap(&w, false,
 * ignore_strand) (genomic_intervals.cpp:5489-5540) for single-interval regions, asked of every window at once.  gtx_window_refs
 * prepares a region set on the device for one scan geometry: ref_triples (host memory, any order, duplicates allowed) are n_refs x
 * (class, start, stop); a region takes part when stop >= 1 and start <= stop, a start below 1 counts as 1; a class id outside
 * [0, n_classes) is GTX_E_RANGE.  class_len, class_offsets, win_step and win_size mean what they mean in gtx_scan: class c has
 * gtx_scan_n_windows(class_len[c], win_step, win_size) windows at class_offsets[c] (offsets in any order; classes that share ordinals, a
 * negative offset and n_refs >= 2^31 - 64 are GTX_E_ARG), window k of it is [win_step k + 1, win_step k + win_size].  n_refs = 0 is a
 * valid set that keeps nothing.  What an earlier call prepared is replaced.
 * gtx_window_filter_device: d_windows is a device vector of n_windows uint64 sums, 16-byte aligned (kept slots are).  A window is kept
 * when its value is >= min_value and a region of its class has start <= the window's stop and stop >= the window's start; ordinals
 * that belong to no class are never kept.  The kept windows come out in vector order: ordinals (int64[capacity]) and values
 * (uint64[capacity]).  *n_kept is the number of kept windows whatever the capacity; when it exceeds capacity only the first `capacity`
 * windows have been written and nothing behind them: grow the buffers and call again (the policy of gtx_window_select).  Before
 * gtx_window_refs: GTX_E_STATE; an unaligned vector, a null output with capacity > 0 or a class that reaches beyond n_windows:
 * GTX_E_ARG.  n_windows = 0 is valid.  The call returns when the result is complete; gtx_window_filter brings it to host memory.
 * Three launches over tiles of GTX_FILTER_TILE windows (count, prefix, emit); a tile no region reaches is not loaded. */
#define GTX_FILTER_TILE 1024
int gtx_window_refs(gtx_ctx *ctx, const int32_t *ref_triples, int64_t n_refs, const int32_t *class_len, const int64_t *class_offsets,
                    int32_t n_classes, int32_t win_step, int32_t win_size);
int gtx_window_filter_device(gtx_ctx *ctx, const void *d_windows, int64_t n_windows, uint64_t min_value, int64_t capacity, void *d_ordinals,
                             void *d_values, int64_t *n_kept);
int gtx_window_filter(gtx_ctx *ctx, const void *d_windows, int64_t n_windows, uint64_t min_value, int64_t capacity, int64_t *ordinals,
                      uint64_t *values, int64_t *n_kept);

/* Peak candidates: the head of the per-window loop of `genomic_scans peaks` (PeakFinder, genomic_scans.cpp:304-311) over window
 * vectors in HBM.  d_signal, d_control and d_uniq (the mappability track; may be NULL) are device vectors of n_windows uint64 window
 * sums, 16-byte aligned (kept slots are), read as signed 64-bit values.  Per window
 *   v0 = d_uniq ? uniq[w] : win_size;   v1 = min(signal[w], v0);   v2 = min(control[w], v0)
 *   norm != 0:  p_ratio < 1.0 ?  v2 = (long)floor((float)v2 * p_ratio)  :  v1 = (long)floor((float)v1 / p_ratio)
 * and the window is kept when v1 >= min_reads.  The conversion to float is the reference's (a count rounds to 24 bits before it is
 * scaled), the product and the quotient are in double.  The kept windows come out in window order: ordinals (int64[capacity]) and rows
 * (int64[capacity * 3]: v1, v2, v0 after clamp and norm).  *n_kept is the number of kept windows whatever the capacity; when it
 * exceeds capacity only the first `capacity` windows have been written and nothing behind them: grow the buffers and call again (the
 * policy of gtx_window_select).  n_windows = 0 is valid.  GTX_E_ARG: a NULL or unaligned signal or control, an unaligned d_uniq, a NULL
 * output with capacity > 0, a negative n_windows or capacity, no n_kept, win_size < 1, or -- with norm set -- a p_ratio that is not
 * finite and positive.  gtx_peak_select_device writes device buffers and returns when the result is complete; gtx_peak_select brings
 * the result to host memory.  Three launches over tiles of GTX_PEAK_TILE windows (count, prefix, emit); the emit pass loads only the
 * tiles that keep a window. */
#define GTX_PEAK_TILE 1024
int gtx_peak_select_device(gtx_ctx *ctx, const void *d_signal, const void *d_control, const void *d_uniq, int64_t n_windows, int64_t win_size,
                           int64_t min_reads, int norm, double p_ratio, int64_t capacity, void *d_ordinals, void *d_rows, int64_t *n_kept);
int gtx_peak_select(gtx_ctx *ctx, const void *d_signal, const void *d_control, const void *d_uniq, int64_t n_windows, int64_t win_size,
                    int64_t min_reads, int norm, double p_ratio, int64_t capacity, int64_t *ordinals, int64_t *rows, int64_t *n_kept);

/* Output lines on the device: what `genomic_scans counts` prints (GenomicRegionSetScanner::PrintRemaining / PrintFiltered), rendered
 * as text from a window vector in HBM or from the (ordinal, value) pairs gtx_window_filter_device left there.
 * gtx_lines_layout uploads the blocks of a scan geometry (host memory): block_offset[n_blocks + 1] ascending from 0 (block b holds
 * the ordinals block_offset[b] .. block_offset[b + 1]; empty blocks share an offset, the last entry is the number of windows), block
 * b's name names_blob[name_off[b] .. name_off[b + 1]) and strand[b] ('+' or '-').  The line of ordinal `at` of block b, with
 * k = at - block_offset[b], is   VALUE '\t' NAME ' ' STRAND ' ' win_step k + 1 ' ' win_step k + win_size '\n'   -- VALUE a signed
 * 64-bit decimal.  GTX_E_ARG: a name longer than GTX_LINES_MAX_NAME (the caller then formats on the host), n_blocks < 1, offsets that
 * do not ascend from 0, a strand that is neither, win_step or win_size < 1, or more than 2^40 windows.  gtx_lines_max_bytes: the
 * longest line that layout can produce (GTX_E_STATE before a layout).
 * gtx_window_lines_device (the vector rule): d_windows is a device vector of uint64 sums, 16-byte aligned, holding at least
 * first + count entries; window i of [first, first + count) is kept when i < limit and (int64) w[i] >= min_value.  The first window
 * in front of `limit` whose value is all-ones is never printed and ends the output whatever min_value is; *end_at is its ordinal, or
 * -1.  The kept lines are written to d_text (device memory, 16-byte aligned) back to back in window order: *n_lines of them, *n_bytes
 * bytes.  GTX_E_ARG when count * gtx_lines_max_bytes exceeds capacity (a caller sizes its ranges by that bound and never repeats a
 * call), for an unaligned pointer, and when first + count reaches beyond the layout's windows.  Nothing is written at or beyond
 * d_text + capacity; bytes between *n_bytes and the next 16-byte boundary are unspecified, what lies behind that boundary is untouched.
 * gtx_pair_lines_device (the pair rule): entries j of [first, first + count) of d_ordinals (int64, ascending) and d_values (uint64),
 * both 16-byte aligned; entry j is kept when 0 <= ordinal[j] < limit and (int64) value[j] >= 0; an all-ones value in front of the
 * limit ends the output (*end_at: its ordinal).
 * Both return when the result is complete.  Count, two prefix scans, emit over tiles of GTX_LINES_TILE entries cut at multiples of
 * GTX_LINES_TILE of the entry index: a tile without a kept line is not loaded again.
 * gtx_window_lines / gtx_pair_lines stream all lines to `sink` in order: ranges of whole tiles, at most gtx_set_lines_chunk bytes of
 * bound each (default 64 MiB; at least one tile's bound is always taken), are rendered into two device buffers in turn, copied into
 * two page-locked buffers and handed to sink(user, text, bytes); range r + 1 renders while r is copied and r - 1 is in the sink.  No
 * line straddles two calls of the sink; a range without a line makes no call.  A sink that returns non-zero ends the call at once
 * with GTX_E_SINK.  The all-ones rule ends the stream.  *n_lines and *n_bytes (either may be NULL) are the totals, *end_at as above.
 * gtx_window_filter_lines is gtx_window_filter_device (after gtx_window_refs) into buffers of the context, then gtx_pair_lines over
 * them: the lines of `genomic_scans counts -r` without the kept ordinals and values crossing to the host. */
#define GTX_E_SINK         -5   /* the caller's sink refused the text */
#define GTX_LINES_TILE 1024
#define GTX_LINES_MAX_NAME 48
typedef int (*gtx_lines_sink)(void *user, const char *text, size_t bytes);
int gtx_lines_layout(gtx_ctx *ctx, const int64_t *block_offset, int32_t n_blocks, const char *names_blob, const int32_t *name_off, const char *strand,
                     int64_t win_step, int64_t win_size);
int64_t gtx_lines_max_bytes(gtx_ctx *ctx);
int gtx_set_lines_chunk(gtx_ctx *ctx, int64_t bytes);
int gtx_window_lines_device(gtx_ctx *ctx, const void *d_windows, int64_t first, int64_t count, int64_t limit, int64_t min_value, void *d_text,
                            int64_t capacity, int64_t *n_lines, int64_t *n_bytes, int64_t *end_at);
int gtx_pair_lines_device(gtx_ctx *ctx, const void *d_ordinals, const void *d_values, int64_t first, int64_t count, int64_t limit, void *d_text,
                          int64_t capacity, int64_t *n_lines, int64_t *n_bytes, int64_t *end_at);
int gtx_window_lines(gtx_ctx *ctx, const void *d_windows, int64_t n_windows, int64_t limit, int64_t min_value, gtx_lines_sink sink, void *user,
                     int64_t *n_lines, int64_t *n_bytes, int64_t *end_at);
int gtx_pair_lines(gtx_ctx *ctx, const void *d_ordinals, const void *d_values, int64_t n, int64_t limit, gtx_lines_sink sink, void *user,
                   int64_t *n_lines, int64_t *n_bytes, int64_t *end_at);
int gtx_window_filter_lines(gtx_ctx *ctx, const void *d_windows, int64_t n_windows, uint64_t min_value, int64_t limit, gtx_lines_sink sink, void *user,
                            int64_t *n_lines, int64_t *n_bytes, int64_t *end_at);

/* genomic_regions win on text (gtools/genomic_regions.cpp:397-403, :647-651, :734; GenomicRegionSet::RunSlidingWindows
 * genomic_intervals.cpp:4449-4455 over GenomicRegionBED::PrintWindows :2520-2532): every line of a block of complete BED lines cut
 * into sliding windows of win_size positions, win_step apart -- what `bedtools makewindows` does.  The block goes to the device as
 * for gtx_rewrite_text (same buffers contract, two blocks in flight, tickets in order).  With START = column 2 + 1, STOP = column 3
 * the windows of a line begin at z = START, START + win_step, .. <= STOP; without `small` the first z with z + win_size - 1 > STOP
 * ends them.  A window prints column 1, TAB, z - 1, TAB, min(z + win_size - 1, STOP), then with 4 or more columns TAB and column 4,
 * with 6 columns TAB column 5 TAB column 6 as well -- a 5-column line loses its score -- and a newline.  A line with START > STOP
 * prints nothing.  The lines the device takes are those of gtx_rewrite_text (the tokenizer's plain case); a block with ANY other
 * line, with a line whose fixed part (column 1, two tabs, the printed columns behind column 3 with their tabs, the newline) is longer
 * than max_fixed of gtx_windows_limits, or with a tile of line_tile consecutive lines whose text is longer than the rewrite's stage,
 * comes back: gtx_windows_result says needs_host, calls no sink and reports zero totals, and the caller renders the block by its own
 * means.  GTX_E_ARG unless 1 <= win_size, win_step <= 2^31 (the caller's own loop takes the rest).
 * gtx_windows_text copies the block in and enqueues the newline index, the tokenizer, the plan of the lines (windows and bytes per
 * line from closed forms of digit counts, nothing loops over windows) and its prefixes.  gtx_windows_result waits for the plan and
 * then streams the block's windows in order to `sink` as gtx_window_lines streams its lines: ranges of whole output tiles of
 * out_tile windows, at most gtx_set_lines_chunk bytes of bound each (a tile's bound is out_tile x (max_fixed + 20); one tile is
 * always taken), range r + 1 rendering while range r is copied.  No line straddles two calls of the sink; a block without a window
 * makes no call (sink may then be NULL).  A sink that returns non-zero ends the call with GTX_E_SINK; the block is dropped and the
 * context stays usable.  *n_windows and *n_bytes (either may be NULL) are the block's totals, equal to what the sink was given.  The
 * result of a ticket must be fetched before the block after next is added.
 * Under gtx_profile_enable a gtx_windows_text call is bracketed as gtx_rewrite_text is (ms_stream_kernel: plan, prefixes and the
 * lines' bases alone on text that is already in HBM), and every range of gtx_windows_result is a profiled call of its own
 * (ms_stream_kernel: the range's emit launch alone). */
typedef struct gtx_windows_op {
  int64_t win_size, win_step;                  /* -s and -d of the reference */
  int32_t small;                               /* --small: the windows that STOP cuts short are printed too */
} gtx_windows_op;
int gtx_windows_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_windows_op *op, int *ticket);
int gtx_windows_result(gtx_ctx *ctx, int ticket, int *needs_host, gtx_lines_sink sink, void *user, int64_t *n_windows /* may be NULL */,
                       int64_t *n_bytes /* may be NULL */);
int gtx_windows_limits(int32_t *line_tile, int32_t *out_tile, int32_t *max_fixed);

/* genomic_regions split | connect | select | diff | n | strand on text (gtools/genomic_regions.cpp:715-716, :721, :728, :732-733): the
 * per-region operations that look inside a region's intervals, which for BED text means inside a 12-column line (a transcript with
 * its exons, a spliced read).  A block of complete BED lines without header lines goes to the device as for gtx_rewrite_text (same
 * buffers contract, two blocks in flight, tickets in order).  With START-1 = column 2, STOP = column 3 and, on a 12-column line,
 * block k at (START-1 + starts[k], START-1 + starts[k] + sizes[k]] (genomic_intervals.cpp:2157-2182):
 *   GTX_BLOCKS_SPLIT    one line per block through the BED PrintModified (:2502-2505, :2310-2314): CHROM TAB the block's START-1 TAB
 *                       its STOP TAB LABEL TAB SCORE TAB STRAND NL.  Always six columns
 *   GTX_BLOCKS_CONNECT  Connect (:1319-1339: one interval from the least start to the greatest stop), UpdateThick (:2326-2333), Print
 *                       (:2188-2218): a 12-column line ends in 1 TAB STOP - (START-1) TAB 0
 *   GTX_BLOCKS_SELECT   Select (:1493-1521) by `select`, bits GTX_BLOCKS_FIRST | LAST | 5P | 3P (5P is the first block on '+' and the
 *                       last on '-', 3P the reverse); UpdateThick; Print.  No bit: nothing is printed.  Both ends: 1 and 2 blocks stay,
 *                       3 or more keep the first and the last.  A line of 3 to 6 columns is its one interval
 *   GTX_BLOCKS_DIFF     Diff (:1345-1361): the gaps between successive blocks as the region's blocks; UpdateThick; Print.  A single
 *                       block, and blocks that all touch, print nothing
 *   GTX_BLOCKS_SIZE     `n` (:1451-1454): LABEL TAB the sum of the blocks' sizes NL, 0 for an interval with start > stop
 *   GTX_BLOCKS_STRAND   ModifyStrand (:1607-1620) by strand_op, GTX_BLOCKS_STRAND_PLUS | MINUS | REVERSE; Print.  A line of fewer than 6
 *                       columns has no column to print the strand into and is printed as it stands
 * Two conventions of this build (the reference prints an unset member there): a 3-column line has the label "_", a line of fewer than
 * 5 columns the score 0 -- where split and n print them.
 * The plain line, which is all the device takes, is one of two kinds.
 * (a) 3 to 6 columns: plain exactly when gtx_rewrite_text calls it plain (above).
 * (b) exactly 12 tab-separated tokens, none empty or holding a byte <= ' '; columns 2, 3, 7, 8 and 10 canonical decimals ("0", or no
 *     leading zero; at most 10 digits); column 5 a canonical long of at most 18 digits; column 6 exactly "+" or "-"; column 10 in
 *     1 .. max_blocks (gtx_blocks_limits: 1024); columns 11 and 12 lists of exactly that many canonical decimals separated by single
 *     commas, with or without one trailing comma; every size >= 1; the first block starts at 0 and the last one ends at column 3 (a
 *     line that does not say so is well defined by Print, but is left to the caller's loop: what Print makes of it is not what the
 *     line holds); every block starts at or behind the end of the block before it (touching blocks are plain, overlapping and
 *     out-of-order ones are not); every coordinate, columns 7 and 8 and the blocks' stops included, below 2^31 - 2.
 * A block with ANY other line -- 7 to 11 columns, blanks as separators, a '.' / '1' / '-1' strand, a count that disagrees with its
 * lists, an input error --, with a line that prints more than 2^25 bytes, or, for the five operations that print one line per line,
 * with a tile of consecutive lines (gtx_blocks_limits) whose output is longer than the stage, comes back: gtx_blocks_result says
 * needs_host, calls no sink and reports zero totals, and the caller renders that block by its own means.  split has no such stage.
 * GTX_E_ARG: a kind that is none of the six, select bits outside the four, a strand_op outside the three.
 * gtx_blocks_text copies the block in and enqueues the newline index (the tokenizer is not run: it calls a 12-column line not plain)
 * and the plan of the lines with its prefixes.  gtx_blocks_result waits for the plan, renders the block and hands the printed lines,
 * in order, to `sink` in calls of at most gtx_set_lines_chunk bytes that end at a line's end; a block that prints nothing (an empty
 * block; select without a bit) makes no call (sink may then be NULL).  A sink that returns non-zero ends the call with GTX_E_SINK;
 * the block is dropped and the context stays usable.  *n_printed and *n_bytes (either may be NULL) are the block's totals.  The result
 * of a ticket must be fetched before the block after next is added.
 * gtx_blocks_max_bytes: a bound on a block's printed bytes for the five operations that print one line per line -- a line's copied
 * columns are its own bytes, and beside them stand at most six rendered coordinates, a count and two fresh list elements of at most
 * 11 bytes for every block of the line, each of which took at least 4 bytes of its input: 7 * bytes + 96 * n_lines.  split prints a
 * line's chromosome and label once per block and has no bound in the block's size: 0, and the plan's own total is what there is.
 * gtx_blocks_limits: the lines per tile of the plan and of the one-line emit, the bytes of such a tile's output that the stage holds,
 * the blocks of a plain line.
 * Under gtx_profile_enable a gtx_blocks_text call is bracketed as gtx_convert_text is (ms_stream_kernel: the plan and its prefixes alone
 * on text that is already in HBM behind its newline index), and the emit launch of gtx_blocks_result is a profiled call of its own. */
#define GTX_BLOCKS_SPLIT   0
#define GTX_BLOCKS_CONNECT 1
#define GTX_BLOCKS_SELECT  2
#define GTX_BLOCKS_DIFF    3
#define GTX_BLOCKS_SIZE    4
#define GTX_BLOCKS_STRAND  5
#define GTX_BLOCKS_FIRST 1
#define GTX_BLOCKS_LAST  2
#define GTX_BLOCKS_5P    4
#define GTX_BLOCKS_3P    8
#define GTX_BLOCKS_STRAND_PLUS    0
#define GTX_BLOCKS_STRAND_MINUS   1
#define GTX_BLOCKS_STRAND_REVERSE 2
typedef struct gtx_blocks_op {
  int32_t kind;                                /* GTX_BLOCKS_SPLIT .. GTX_BLOCKS_STRAND */
  int32_t select;                              /* GTX_BLOCKS_SELECT: bits GTX_BLOCKS_FIRST | LAST | 5P | 3P */
  int32_t strand_op;                           /* GTX_BLOCKS_STRAND: GTX_BLOCKS_STRAND_PLUS | MINUS | REVERSE */
} gtx_blocks_op;
int gtx_blocks_text(gtx_ctx *ctx, const char *text, size_t bytes, int64_t n_lines, const gtx_blocks_op *op, int *ticket);
int gtx_blocks_result(gtx_ctx *ctx, int ticket, int *needs_host, gtx_lines_sink sink, void *user, int64_t *n_printed /* may be NULL */,
                      int64_t *n_bytes /* may be NULL */);
size_t gtx_blocks_max_bytes(size_t bytes, int64_t n_lines, const gtx_blocks_op *op);
int gtx_blocks_limits(int32_t *tile, int32_t *stage, int32_t *max_blocks);

/* ---- measurement ------------------------------------------------------------------------ */

/* on = 1: every *_device call brackets its dominant kernel and the whole call with HIP events on the
 * context's stream (three records, ~5 us of stream bubble each on this platform).
 * on = N >= 2: only every N-th call is profiled and only its dominant kernel is bracketed (two records;
 * ms_total then repeats ms_stream_kernel) -- for timing loops that should not be stretched by their own
 * instrumentation.  on = 0: off.  Resets the ring of profiled calls. */
int gtx_profile_enable(gtx_ctx *ctx, int on);
/* Elapsed ms of the last profiled call: the streaming kernel alone, and the whole enqueue
 * (memsets + stream kernel + finalize kernels).  Waits for that call to finish. */
int gtx_profile_last(gtx_ctx *ctx, float *ms_stream_kernel, float *ms_total);
/* Same for the call `back` calls before the last one (0 = last); the last 64 profiled calls
 * are kept, so a timed loop can be read back after it ends without synchronising inside it. */
int gtx_profile_read(gtx_ctx *ctx, int back, float *ms_stream_kernel, float *ms_total);
/* How many profiled calls gtx_profile_read can reach (<= 64) since the last gtx_profile_enable. */
int gtx_profile_count(gtx_ctx *ctx);

/* Library/ABI version, e.g. 100 = 1.0.0 */
int gtx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GTX_H */
