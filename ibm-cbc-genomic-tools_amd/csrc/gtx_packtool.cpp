// gtx_packtool -- host-only view of the BED ingest (gtx_bed.*): packs a BED stream with the rules of one
// of the four consumers and prints the packed triples as text.  No GPU, no libgtx: this is how the
// CPU test suite checks the packer (line handling, tokenising, order checks, error text and line numbers,
// thread-count independence) on machines without an MI355X.
//
//   gtx_packtool MODE [-t THREADS] [-s] [-a] [-l MAXLABEL] [--sam | --gff] [-c CHROM,CHROM,...] [FILE]
//     MODE   ou = overlaps/unsorted   os = overlaps/sorted   su = scan/unsorted   ss = scan/sorted
//     -g / -m / -e   multi-interval regions: on their envelope (-gaps) / listed (count) / one read per interval (coverage)
//     --sam  the file is SAM: its '@' header lines are skipped (they keep their line numbers; FILE only), the alignments read as
//            GenomicRegionSAM does; a spliced read's intervals are printed as "# blocks class start end n s1 e1 s2 e2 ..."
//     --gff  the file is GFF / GTF: its leading '##' lines are skipped (they keep their line numbers; FILE only), the features read as
//            GenomicRegionGFF does; with -a a strand byte other than '+' or '-' is an error.  (`pack` takes no GFF.)
//     -s sorted by strand   -a strand-aware classes   -c known chromosomes (default: all seen in FILE order? no:
//        the list is required for reproducible class ids)
//   output: one line per packed read "class start end [weight]", then "# lines=N"; errors like the CLIs.
//
//   gtx_packtool route [RULE ARG...]   the library's kernel-route rules (gtx_routes.h), see RouteQuery below
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "gtx_bed.h"
#include "gtx_stats.h"
#include "gtx_peakdiff.h"
#include "gtx_routes.h"

using namespace gtxhost;

// ---- synthetic BED files (the workload of SURVEY 8(d): hg38 chromosome lengths) -------------------------------------------
#include <algorithm>
#include <thread>
#include <vector>
static int SynthBed(bool refs, long long n, unsigned long long seed, const char *out_path, long read_len, bool sam = false, bool gff = false)
{
  static const struct { const char *name; long len; } chr[24] = {   // strcmp order
    {"chr1", 248956422}, {"chr10", 133797422}, {"chr11", 135086622}, {"chr12", 133275309}, {"chr13", 114364328}, {"chr14", 107043718},
    {"chr15", 101991189}, {"chr16", 90338345}, {"chr17", 83257441}, {"chr18", 80373285}, {"chr19", 58617616}, {"chr2", 242193529},
    {"chr20", 64444167}, {"chr21", 46709983}, {"chr22", 50818468}, {"chr3", 198295559}, {"chr4", 190214555}, {"chr5", 181538259},
    {"chr6", 170805979}, {"chr7", 159345973}, {"chr8", 145138636}, {"chr9", 138394717}, {"chrX", 156040895}, {"chrY", 57227415}};
  double total = 0; for (auto &c : chr) total += (double)c.len;
  std::vector<long long> per(24); long long given = 0;
  for (int c = 0; c < 24; c++) { per[c] = (long long)((double)n * chr[c].len / total); given += per[c]; }
  for (int c = 0; given < n; c = (c + 1) % 24) { per[c]++; given++; }
  std::vector<long long> first(25, 0);
  for (int c = 0; c < 24; c++) first[c + 1] = first[c] + per[c];
  std::vector<std::string> text(24);
  auto make = [&](int c) {
    unsigned long long x = seed * 0x9E3779B97F4A7C15ull + (unsigned long long)(c + 1) * 0xBF58476D1CE4E5B9ull;
    auto next = [&x]() { x += 0x9E3779B97F4A7C15ull; unsigned long long z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
    const long long k = per[c];
    std::vector<unsigned> s((size_t)k), ln(refs ? (size_t)k : 0);
    const unsigned long long span = (unsigned long long)(chr[c].len - (refs ? 2001 : read_len + 1));
    for (long long i = 0; i < k; i++) s[(size_t)i] = (unsigned)(next() % span);
    std::sort(s.begin(), s.end());
    if (refs) for (long long i = 0; i < k; i++) ln[(size_t)i] = 50 + (unsigned)(next() % 1950);
    std::string &t = text[c];
    t.reserve((size_t)k * (refs ? 40 : sam ? (size_t)(2 * read_len + 100) : gff ? 130 : 30));
    if (sam) {                                                    // SAM: the same reads as alignments, r<i> FLAG 0|16 ... <LEN>M
      static const char base[4] = {'A', 'C', 'G', 'T'};
      std::string seq((size_t)read_len, 'A'), qual((size_t)read_len, 'F');
      char head[160];
      for (long long i = 0; i < k; i++) {
        for (long b = 0; b < read_len; b++) seq[(size_t)b] = base[(next() >> 7) & 3];
        const unsigned flag = (next() & 1) ? 16u : 0u;
        int h = snprintf(head, sizeof head, "r%lld\t%u\t%s\t%u\t60\t%ldM\t*\t0\t0\t", first[c] + i, flag, chr[c].name, s[(size_t)i] + 1, read_len);
        t.append(head, (size_t)h); t += seq; t += '\t'; t += qual;
        h = snprintf(head, sizeof head, "\tNM:i:0\tMD:Z:%ld\tAS:i:%ld\n", read_len, read_len);
        t.append(head, (size_t)h);
      }
      return;
    }
    if (gff) {                                                    // GTF: the same reads as exon features, 9 columns, an attribute string for a label
      char line[256];
      for (long long i = 0; i < k; i++) {
        const long long id = first[c] + i;
        const int h = snprintf(line, sizeof line, "%s\tsynth\texon\t%u\t%llu\t.\t%c\t.\tgene_id \"G%lld\"; transcript_id \"T%lld.1\"; exon_number \"%d\";\n",
                               chr[c].name, s[(size_t)i] + 1, (unsigned long long)s[(size_t)i] + (unsigned long long)read_len, (next() & 1) ? '-' : '+', id / 7, id / 3, (int)(id % 3) + 1);
        t.append(line, (size_t)h);
      }
      return;
    }
    char buf[96];
    const size_t nl = strlen(chr[c].name);
    for (long long i = 0; i < k; i++) {
      char *p = buf; memcpy(p, chr[c].name, nl); p += nl; *p++ = '\t';
      auto put = [&p](unsigned long long v) { char tmp[24]; int d = 0; do { tmp[d++] = (char)('0' + v % 10); v /= 10; } while (v); while (d) *p++ = tmp[--d]; };
      put(s[(size_t)i]); *p++ = '\t'; put((unsigned long long)s[(size_t)i] + (refs ? ln[(size_t)i] : (unsigned long long)read_len));
      if (refs) { *p++ = '\t'; *p++ = 'g'; put((unsigned long long)(first[c] + i)); }
      *p++ = '\n';
      t.append(buf, (size_t)(p - buf));
    }
  };
  {
    std::vector<std::thread> th;
    for (int c = 0; c < 24; c++) th.emplace_back(make, c);
    for (auto &x : th) x.join();
  }
  FILE *o = fopen(out_path, "wb");
  if (!o) { fprintf(stderr, "Error: cannot create file '%s'!\n", out_path); return 1; }
  if (sam) {
    fprintf(o, "@HD\tVN:1.6\tSO:coordinate\n");
    for (int c = 0; c < 24; c++) fprintf(o, "@SQ\tSN:%s\tLN:%ld\n", chr[c].name, chr[c].len);
  }
  if (gff) fprintf(o, "##gff-version 2\n##source-version gtx_packtool synthgff\n");
  for (int c = 0; c < 24; c++) if (fwrite(text[c].data(), 1, text[c].size(), o) != text[c].size()) { fprintf(stderr, "Error: cannot write file '%s'!\n", out_path); return 1; }
  return fclose(o) == 0 ? 0 : 1;
}

// One query of `gtx_packtool route`: a rule of gtx_routes.h by name with its arguments in the rule's own order, the knobs from the
// environment as the library reads them (RouteKnobs::from_env).  Prints the result on one line; false: not a query.
//   finalize NB NBRUN SUMSVALID HAVECHAIN HAVETOTALS LOCALMAXTILES -> gather_only | sums_kept | chained | local | sums_scan
//   keeps_tile_sums HISTLEN NREADS      flip REGIONS NREADS      hist32 SINGLEUNWEIGHTEDLAUNCH NREADS      partition_worth N BUCKETMINREADS
//   count_cpw NREADS WAVESLOTS FORCED   cover_cpw NREADS FORCED  scan_per TOTALMICRO PARTBINS              scan_tables_ok NB NCLASSES TOTALMICRO
//   scan_own READSSORTED PREPONE NREADS scan_fused COMB MAXCOMB TOTALWINDOWS                               scan_tiles LEN
static bool RouteQuery(const char *line)
{
  static const char *const fin[] = {"gather_only", "sums_kept", "chained", "local", "sums_scan"};
  const gtx::RouteKnobs k = gtx::RouteKnobs::from_env();
  char rule[32]; long long a[6] = {0, 0, 0, 0, 0, 0};
  const int n = sscanf(line, " %31s %lld %lld %lld %lld %lld %lld", rule, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) - 1;
  const std::string r = n >= 0 ? rule : "";
  if (r == "finalize" && n == 6) printf("%s\n", fin[gtx::finalize_route((int)a[0], (int)a[1], a[2] != 0, a[3] != 0, a[4] != 0, (int)a[5], k)]);
  else if (r == "keeps_tile_sums" && n == 2) printf("%d\n", (int)gtx::keeps_tile_sums(a[0], a[1], k));
  else if (r == "flip" && n == 2) printf("%d\n", (int)gtx::flip_walk(a[0], a[1], k));
  else if (r == "hist32" && n == 2) printf("%d\n", (int)gtx::hist32_slots(a[0] != 0, a[1], k));
  else if (r == "partition_worth" && n == 2) printf("%d\n", (int)gtx::partition_worth(a[0], a[1]));
  else if (r == "count_cpw" && n == 3) printf("%d\n", gtx::count_chunks_per_wave(a[0], a[1], (int)a[2]));
  else if (r == "cover_cpw" && n == 2) printf("%d\n", gtx::cover_chunks_per_wave(a[0], (int)a[1]));
  else if (r == "scan_per" && n == 2) printf("%lld\n", gtx::scan_bucket_per(a[0], (int)a[1], k));
  else if (r == "scan_tables_ok" && n == 3) printf("%d\n", (int)gtx::scan_bucket_tables_ok(a[0], (int)a[1], a[2]));
  else if (r == "scan_own" && n == 3) printf("%d\n", (int)gtx::scan_own_wanted(a[0] != 0, a[1] != 0, a[2], k));
  else if (r == "scan_fused" && n == 3) printf("%d\n", (int)gtx::scan_fused_ok((int)a[0], (int)a[1], a[2], k));
  else if (r == "scan_tiles" && n == 1) printf("%d\n", gtx::scan_tiles(a[0]));
  else return false;
  return true;
}

int main(int argc, char **argv)
{
  if (argc < 2) { fprintf(stderr, "usage: gtx_packtool ou|os|su|ss [-t N] [-s] [-a] [-l MAX] -c chr1,chr2,... [FILE]\n"); return 2; }
  PackOptions opt;
  std::string m = argv[1];
  if (m == "pack") {
    // gtx_packtool pack [--sam] IN.bed[.gz] OUT.gtx : tokenise once, keep the columns (gtx_bed.h, "packed region files")
    const bool sam = argc == 5 && !strcmp(argv[2], "--sam");
    if (argc != 4 && !sam) { fprintf(stderr, "usage: gtx_packtool pack [--sam] IN.bed OUT.gtx\n"); return 2; }
    std::string err;
    LineSource *src = LineSource::Open(argv[sam ? 3 : 2], &err);
    if (!src) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    PackError e;
    if (!WriteGtx(src, argv[sam ? 4 : 3], &e, sam)) {
      if (e.no_prefix) fprintf(stderr, "%s\n", e.msg.c_str()); else fprintf(stderr, "\nError: Line %ld: %s\n", e.line, e.msg.c_str());
      return 1;
    }
    delete src;
    return 0;
  }
  if (m == "synth" || m == "synthrefs") {
    // gtx_packtool synth N SEED OUT.bed [LEN]      N reads of LEN bp (default 50) on the 24 hg38 chromosomes, in proportion to their
    //                                              length, sorted by (chromosome in strcmp order, start), BED3
    // gtx_packtool synthrefs M SEED OUT.bed        M regions of 50..2000 bp, same order, BED4 with labels g0, g1, ...
    // Workload files for the end-to-end timings (bench.py text_to_stdout): written by a thread per chromosome, ~1 GB/s.
    if (argc < 5) { fprintf(stderr, "usage: gtx_packtool synth|synthrefs N SEED OUT.bed [LEN]\n"); return 2; }
    return SynthBed(m == "synthrefs", atoll(argv[2]), strtoull(argv[3], NULL, 10), argv[4], argc > 5 ? atol(argv[5]) : 50);
  }
  if (m == "synthsam") {
    // gtx_packtool synthsam N SEED OUT.sam [LEN]   the reads of `synth` as SAM alignments: a header, QNAME r<i>, FLAG 0 or 16, MAPQ 60,
    //                                              CIGAR <LEN>M, SEQ and QUAL of LEN bases, three optional tags (lines of ~2.5 LEN + 80 bytes)
    if (argc < 5) { fprintf(stderr, "usage: gtx_packtool synthsam N SEED OUT.sam [LEN]\n"); return 2; }
    return SynthBed(false, atoll(argv[2]), strtoull(argv[3], NULL, 10), argv[4], argc > 5 ? atol(argv[5]) : 100, true);
  }
  if (m == "synthgff") {
    // gtx_packtool synthgff N SEED OUT.gtf [LEN]   the reads of `synth` as GTF exon features: a '##' header, 9 columns, strand + or -, an
    //                                              attribute string (gene_id, transcript_id, exon_number) as the label (lines of ~100 bytes)
    if (argc < 5) { fprintf(stderr, "usage: gtx_packtool synthgff N SEED OUT.gtf [LEN]\n"); return 2; }
    return SynthBed(false, atoll(argv[2]), strtoull(argv[3], NULL, 10), argv[4], argc > 5 ? atol(argv[5]) : 100, false, true);
  }
  if (m == "stats") {
    // the host-side tail probabilities of `genomic_scans peaks` (gtx_stats.h), one "b K P N" / "p K MU" / "g X" query per stdin line
    char kind; double x, y, z;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
      int n = sscanf(line, " %c %lf %lf %lf", &kind, &x, &y, &z);
      if (n >= 4 && kind == 'b') printf("%.17g\n", gtxstats::BinomialQ((long)x, y, (long)z));
      else if (n >= 3 && kind == 'p') printf("%.17g\n", gtxstats::PoissonQ((long)x, y));
      else if (n >= 2 && kind == 'g') printf("%.17g\n", gtxstats::GaussianQ(x));
      else { fprintf(stderr, "bad query: %s", line); return 2; }
    }
    return 0;
  }
  if (m == "route") {
    // gtx_packtool route RULE ARG... : one query from the command line; gtx_packtool route : one query per stdin line
    std::string q;
    for (int a = 2; a < argc; a++) { q += argv[a]; q += ' '; }
    char line[256];
    if (argc > 2) { if (!RouteQuery(q.c_str())) { fprintf(stderr, "bad query: %s\n", q.c_str()); return 2; } return 0; }
    while (fgets(line, sizeof line, stdin)) if (!RouteQuery(line)) { fprintf(stderr, "bad query: %s", line); return 2; }
    return 0;
  }
  if (m == "critical") {
    // gtx_packtool critical P W CUTOFF CONTROL : peakdiff's table of critical counts (gtx_peakdiff.h), one per line -- W + 1 lines
    // with CONTROL = 1 (one per control count), one line with CONTROL = 0
    if (argc != 6) { fprintf(stderr, "usage: gtx_packtool critical P W CUTOFF CONTROL\n"); return 2; }
    const long W = atol(argv[3]);
    if (W < 1) { fprintf(stderr, "bad window size: %s\n", argv[3]); return 2; }
    for (int k : gtxstats::CriticalCounts(atof(argv[2]), W, atof(argv[4]), atoi(argv[5]) != 0)) printf("%d\n", k);
    return 0;
  }
  if (m == "ou") opt.mode = PACK_OVERLAPS_UNSORTED; else if (m == "os") opt.mode = PACK_OVERLAPS_SORTED;
  else if (m == "su") opt.mode = PACK_SCAN_UNSORTED; else if (m == "ss") opt.mode = PACK_SCAN_SORTED;
  else { fprintf(stderr, "unknown mode '%s'\n", argv[1]); return 2; }
  ChromTable chroms;
  const char *file = NULL; size_t batch = 1u << 20;
  bool quiet = false; long long checksum = 0, n_reads = 0;                    // -q: timing runs, print only a checksum
  for (int a = 2; a < argc; a++) {
    if (!strcmp(argv[a], "-t") && a + 1 < argc) opt.threads = atoi(argv[++a]);
    else if (!strcmp(argv[a], "-s")) opt.sorted_by_strand = true;
    else if (!strcmp(argv[a], "-a")) opt.strand_aware = true;
    else if (!strcmp(argv[a], "-z")) opt.collect_zero_length = true;
    else if (!strcmp(argv[a], "-q")) quiet = true;
    else if (!strcmp(argv[a], "--sam")) opt.sam = true;
    else if (!strcmp(argv[a], "--gff")) opt.gff = true;
    else if (!strcmp(argv[a], "-g")) opt.match_gaps = true;           // -gaps: a multi-interval region on its envelope
    else if (!strcmp(argv[a], "-m")) opt.collect_blocks = true;       // count without -gaps: multi-interval regions on their own list
    else if (!strcmp(argv[a], "-e")) opt.explode_blocks = true;       // coverage without -gaps: every interval a read of its own
    else if (!strcmp(argv[a], "-l") && a + 1 < argc) opt.max_label_value = atol(argv[++a]);
    else if (!strcmp(argv[a], "-b") && a + 1 < argc) batch = (size_t)atol(argv[++a]);
    else if (!strcmp(argv[a], "-c") && a + 1 < argc) {
      std::string list = argv[++a];
      size_t p = 0;
      while (p <= list.size()) { size_t q = list.find(',', p); if (q == std::string::npos) q = list.size(); if (q > p) chroms.Add(list.substr(p, q - p).c_str()); p = q + 1; }
    } else file = argv[a];
  }
  chroms.Freeze();
  opt.chroms = &chroms;
  std::string err;
  LineSource *src = nullptr; GtxView *packed = nullptr;
  if (GtxView::IsGtx(file)) { packed = GtxView::Open(file, &err); if (!packed) { fprintf(stderr, "%s\n", err.c_str()); return 1; } }
  else { src = LineSource::Open(file, &err); if (!src) { fprintf(stderr, "%s\n", err.c_str()); return 1; } }
  BedPacker packer_text(src, opt), packer_packed(packed, opt);
  BedPacker &packer = packed ? packer_packed : packer_text;
  if (opt.sam && opt.gff) { fprintf(stderr, "--sam and --gff exclude each other\n"); return 2; }
  if ((opt.sam || opt.gff) && src && file) {                 // the '@' / '##' header is skipped (its lines counted): a first look counts them
    long h = 0;
    LineSource *peek = LineSource::Open(file, &err);
    for (char *l = peek ? peek->Next() : NULL; l && (opt.sam ? l[0] == '@' : (l[0] == '#' && l[1] == '#')); l = peek->Next()) h++;
    delete peek;
    for (long k = 0; k < h; k++) src->Next();
  }
  PackedBatch b; PackError e; int64_t lines = 0;
  for (;;) {
    bool more = packer.NextBatch(&b, batch, &e);
    if (e.set) {
      fflush(stdout);
      if (e.no_prefix) fprintf(stderr, "%s\n", e.msg.c_str()); else fprintf(stderr, "\nError: Line %ld: %s\n", e.line, e.msg.c_str());
      return 1;
    }
    if (quiet) { long long cs = 0; for (size_t i = 0; i < b.tri.size(); i++) cs += b.tri[i]; checksum += cs; n_reads += (long long)(b.tri.size() / 3); b.tri.clear(); b.w.clear(); b.zero_len.clear(); lines += b.n_lines; b.n_lines = 0; if (!more) break; continue; }
    for (size_t i = 0; i + 2 < b.tri.size(); i += 3) {
      if (b.w.empty()) printf("%d %d %d\n", b.tri[i], b.tri[i + 1], b.tri[i + 2]);
      else printf("%d %d %d %d\n", b.tri[i], b.tri[i + 1], b.tri[i + 2], b.w[i / 3]);
    }
    for (size_t i = 0; i + 2 < b.zero_len.size(); i += 3) printf("# zero %d %d %d\n", b.zero_len[i], b.zero_len[i + 1], b.zero_len[i + 2]);
    for (size_t i = 0, at = 0; i < b.m_cnt.size(); i++) {
      printf("# blocks %d %d %d %d", b.m_tri[3 * i], b.m_tri[3 * i + 1], b.m_tri[3 * i + 2], b.m_cnt[i]);
      for (int k = 0; k < 2 * b.m_cnt[i]; k++) printf(" %d", b.m_blocks[at++]);
      printf("\n");
    }
    lines += b.n_lines;
    if (!more) break;
  }
  if (quiet) printf("# reads=%lld checksum=%lld\n", n_reads, checksum);
  printf("# lines=%ld\n", (long)lines);
  delete src; delete packed;
  return 0;
}
