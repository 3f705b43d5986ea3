// genomic_peakdiff -- MI355X edition of the data pass of GenomicTools' `genomic_apps peakdiff` (reference driver:
// gtools/genomic_apps.cpp:179-200 options, :669-743 the operation, :314-431 ScanReadFiles).  Same command line behind the operation
// word, same PREFIX.params and PREFIX.dat, same errors.  Every read file goes through an UnsortedGenomicRegionSetScanner (preprocess
// 'c') whose windows stay in HBM (KeepNextOnDevice); the reference's per-window binomial tail is folded into tables of critical counts
// (gtx_peakdiff.h) and the windows are chosen on the device (GtxSelectWindows: gtx_window_select), so only the kept windows and their
// counts come to the host.  `genomic_apps peakdiff` itself stays refused (genomic_apps.cpp of this package).
//
// The steps behind the data pass are not part of this build: the reference writes an R script (quantile normalisation, outlier
// removal, fold changes, plots) and runs `R CMD BATCH` on it.  Here the `-R` file must still exist (the reference's check), no
// PREFIX.r is written and nothing is run; one line on stderr says so.  `-reuse` therefore only rewrites PREFIX.params.  One GPU.
// Where the reference's GSL aborts on a background probability above 1 (more regions than genome positions), this tool prints an
// error and exits.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"
#include "gtx_peakdiff.h"

static const char *PROGRAM = "genomic_peakdiff";
static const long int BUFFER_SIZE = 10000;

// CountTokens / GetNextToken / Tokenize (core.cpp:577-625, genomic_apps.cpp:250-260): NULL or "" has no tokens
static std::vector<std::string> Tokenize(const char *s, char delim)
{
  std::vector<std::string> out;
  if (s == NULL || s[0] == 0) return out;
  const char *p = s;
  for (;;) {
    while (*p == ' ') p++;
    if (*p == 0) return out;
    const char *e = p;
    while (*e && *e != delim) e++;
    out.push_back(std::string(p, (size_t)(e - p)));
    if (*e == 0) return out;
    p = e + 1;
  }
}

static FILE *OpenOut(const std::string &name)
{
  FILE *f = fopen(name.c_str(), "w");
  if (f == NULL) { fprintf(stderr, "Error: cannot open file '%s' for writing!\n", name.c_str()); exit(1); }
  return f;
}

// one read file: its set, its scanner with the windows kept in a slot of the device context, its background probability (:329-332)
struct ReadFile {
  GenomicRegionSet *set;
  UnsortedGenomicRegionSetScanner *scanner;
  double p;
};

int main(int argc, char *argv[])
{
  GtxAcceptGFF(false);                                        // (GFF input stays unsupported here; SAM is read as before)
  bool HELP, HELP2, VERBOSE, REUSE, IGNORE_STRAND;
  const char *RSCRIPT, *OUT_PREFIX, *GENOME_REG_FILE, *SCALING, *NORMALIZATION, *LABELS, *IMAGE_TYPE, *IMAGE_SIZE;
  long MAX_LABEL_VALUE, WIN_SIZE, WIN_DIST, FDR_BINS, IMAGE_RESOLUTION;
  double PVALUE_CUTOFF, OUTLIER_PROB, PSEUDOCOUNT, FDR, FOLD_CUTOFF;
  gtxhost::Options opts;                                                    // :150-152, :181-200, in the reference's order
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  opts.Flag("-reuse", &REUSE, "reuse histogram data; update paramaters only");
  opts.Str("-R", &RSCRIPT, "", "R script file to use (not required)");
  opts.Str("-o", &OUT_PREFIX, "", "prefix for output files (required)");
  opts.Flag("-i", &IGNORE_STRAND, "ignore strand while finding overlaps");
  opts.Str("-g", &GENOME_REG_FILE, "", "genome region file");
  opts.Long("--max-label-value", &MAX_LABEL_VALUE, 1, "maximum input region label value to be used");
  opts.Long("-w", &WIN_SIZE, 500, "window size (must be a multiple of window distance)");
  opts.Long("-d", &WIN_DIST, 100, "window distance");
  opts.Double("-pval", &PVALUE_CUTOFF, 1.0e-05, "p-value cutoff for calling significant windows");
  opts.Double("-outliers", &OUTLIER_PROB, 0.01, "probability cutoff for residuals in outlier detection between replicates");
  opts.Str("-scale", &SCALING, "winsize", "scaling type: 'winsize' to scale by window size, or 'none'");
  opts.Str("-norm", &NORMALIZATION, "normq", "normalization type: 'normq' for quantile normalization, or 'none'");
  opts.Double("-pseudo", &PSEUDOCOUNT, 1.0, "pseudocount to be added to window count for fold-change computations");
  opts.Long("-nbins", &FDR_BINS, 1, "number of bins for binned FDR computation");
  opts.Double("-fdr", &FDR, 0.05, "false discover rate for differential peak discovery");
  opts.Double("-fold", &FOLD_CUTOFF, 1.00, "adjusted fold change cutoff for gain and loss output files");
  opts.Str("-labels", &LABELS, "", "comma-separated sample labels (required)");
  opts.Str("-itype", &IMAGE_TYPE, "pdf", "image format type {pdf,tif}");
  opts.Str("-isize", &IMAGE_SIZE, "3000,2000", "comma-separated image dimensions (for tif format only)");
  opts.Long("-ires", &IMAGE_RESOLUTION, 300, "image resolution in dpi (for tif format only)");
  const int next_arg = opts.Parse(argc, argv, 1);
  if (HELP || HELP2 || argc - next_arg < 2) {
    opts.Usage(PROGRAM, "[OPTIONS]", "SAMPLE1-FILES SAMPLE2-FILES [SAMPLE1-CONTROL-FILES SAMPLE2-CONTROL-FILES]");
    return 1;
  }
  if (strcmp(IMAGE_TYPE, "pdf") != 0 && strcmp(IMAGE_TYPE, "tif") != 0) { fprintf(stderr, "Error: unsupported image format '%s'!\n", IMAGE_TYPE); return 1; }
  _MESSAGES_ = VERBOSE;

  // :670-690
  if (strlen(OUT_PREFIX) == 0) { fprintf(stderr, "Error: prefix for output files must be specified using the -o option!\n"); return 1; }
  const std::vector<std::string> signal_file = Tokenize(argv[next_arg], ','), ref_file = Tokenize(argv[next_arg + 1], ',');
  const int n_signal = (int)signal_file.size(), n_ref = (int)ref_file.size();
  if (n_signal > 2 || n_ref > 2) { fprintf(stderr, "Error: this method requires at most two replicates per sample!\n"); return 1; }
  const std::vector<std::string> signal_control_file = Tokenize(argc > next_arg + 2 ? argv[next_arg + 2] : NULL, ','),
                                 ref_control_file = Tokenize(argc > next_arg + 3 ? argv[next_arg + 3] : NULL, ',');
  const int n_signal_control = (int)signal_control_file.size(), n_ref_control = (int)ref_control_file.size();
  if (n_signal_control > 0 && (n_signal_control != n_signal || n_ref_control != n_ref)) {
    fprintf(stderr, "Error: number of control files should match the number of signal files for each sample!\n"); return 1;
  }
  const std::vector<std::string> labels = Tokenize(LABELS, ',');
  if (labels.size() != 2) { fprintf(stderr, "Error: please supply labels for each sample using the -labels option!\n"); return 1; }

  // :693-720
  const std::string data_file_name = std::string(OUT_PREFIX) + ".dat", param_file_name = std::string(OUT_PREFIX) + ".params";
  FILE *param_file = OpenOut(param_file_name);
  fprintf(param_file, "n_signal %d\n", n_signal);
  fprintf(param_file, "n_ref %d\n", n_ref);
  fprintf(param_file, "win %ld\n", WIN_SIZE);
  fprintf(param_file, "pval %.6e\n", PVALUE_CUTOFF);
  fprintf(param_file, "scale %s\n", SCALING);
  fprintf(param_file, "norm %s\n", NORMALIZATION);
  fprintf(param_file, "pseudo %.6e\n", PSEUDOCOUNT);
  fprintf(param_file, "outliers %.6e\n", OUTLIER_PROB);
  fprintf(param_file, "fdr %.6e\n", FDR);
  fprintf(param_file, "fold %.6e\n", FOLD_CUTOFF);
  fprintf(param_file, "fdr_bins %ld\n", FDR_BINS);
  fprintf(param_file, "labels %s\n", LABELS);
  fprintf(param_file, "isize %s\n", IMAGE_SIZE);
  fprintf(param_file, "ires %d\n", (int)IMAGE_RESOLUTION);
  fprintf(param_file, "# ");
  for (int i = 0; i < argc; i++)
    if (strchr(argv[i], ' ') == NULL) fprintf(param_file, "%s%c", argv[i], i < argc - 1 ? ' ' : '\n');
    else fprintf(param_file, "'%s'%c", argv[i], i < argc - 1 ? ' ' : '\n');
  fclose(param_file);

  if (!REUSE) {                                                             // ScanReadFiles (:314-431)
    if (WIN_SIZE < 1) { fprintf(stderr, "Error: window size must be positive!\n"); return 1; }
    StringLIntMap *bounds = ReadBounds((char *)GENOME_REG_FILE);
    const unsigned long int effective_genome_size = CalcBoundSize(bounds);
    if (VERBOSE) fprintf(stderr, "* Effective genome size = %lu\n", effective_genome_size);
    // the files in the order of the .dat columns: sample 1, sample 2, sample 1's controls, sample 2's controls
    std::vector<ReadFile> files;
    auto open_files = [&](const std::vector<std::string> &names, const char *what) {
      for (const std::string &name : names) {
        ReadFile f;
        f.set = new GenomicRegionSet((char *)name.c_str(), BUFFER_SIZE, VERBOSE, false, true);
        GenomicRegionSetScanner::KeepNextOnDevice((int)files.size());
        f.scanner = new UnsortedGenomicRegionSetScanner(f.set, bounds, WIN_DIST, WIN_SIZE, MAX_LABEL_VALUE, IGNORE_STRAND, 'c');
        // CountGenomicRegions(file, false): every region counts 1 -- the scan's own label sum when the labels are not used
        const long int n_regions = MAX_LABEL_VALUE <= 1 ? f.scanner->TotalLabelValue() : CountGenomicRegions((char *)name.c_str(), 0);
        f.p = (double)n_regions / effective_genome_size;
        if (VERBOSE) fprintf(stderr, "* %s input file = %s; background probability = %.2e\n", what, name.c_str(), f.p);
        if (!(f.p <= 1.0)) {
          fprintf(stderr, "Error: background probability of '%s' is above 1: %ld regions on %lu genome positions!\n", name.c_str(), n_regions, effective_genome_size);
          exit(1);
        }
        files.push_back(f);
      }
    };
    open_files(signal_file, "Signal");
    open_files(signal_control_file, "Signal control");
    open_files(ref_file, "Reference");
    open_files(ref_control_file, "Reference control");
    // (opened in the reference's order, :328-366; the columns are sample 1, sample 2, then the controls)
    std::vector<ReadFile> order;
    for (int s = 0; s < n_signal; s++) order.push_back(files[(size_t)s]);
    for (int r = 0; r < n_ref; r++) order.push_back(files[(size_t)(n_signal + n_signal_control + r)]);
    for (int s = 0; s < n_signal_control; s++) order.push_back(files[(size_t)(n_signal + s)]);
    for (int r = 0; r < n_ref_control; r++) order.push_back(files[(size_t)(n_signal + n_signal_control + n_ref + r)]);
    const int n_tested = n_signal + n_ref, n_control = n_signal_control + n_ref_control;

    FILE *out_file = OpenOut(data_file_name);
    fprintf(out_file, "locus");
    for (int s = 0; s < n_signal; s++) fprintf(out_file, "\t%s count %d", labels[0].c_str(), s + 1);
    for (int r = 0; r < n_ref; r++) fprintf(out_file, "\t%s count %d", labels[1].c_str(), r + 1);
    for (int s = 0; s < n_signal_control; s++) fprintf(out_file, "\t%s control count %d", labels[0].c_str(), s + 1);
    for (int r = 0; r < n_ref_control; r++) fprintf(out_file, "\t%s control count %d", labels[1].c_str(), r + 1);
    fprintf(out_file, "\n");

    if (n_tested > 0) {                                                     // (no sample 1 file: the reference's loop reads signal_val[0] unset)
      std::vector<GenomicRegionSetScanner *> scanners;
      std::vector<std::vector<int> > tables;
      for (const ReadFile &f : order) scanners.push_back(f.scanner);
      for (int f = 0; f < n_tested; f++) tables.push_back(gtxstats::CriticalCounts(order[(size_t)f].p, WIN_SIZE, PVALUE_CUTOFF, n_control > 0));
      std::vector<long long> ordinals; std::vector<int> rows; std::string error;
      if (!GtxSelectWindows(scanners.data(), n_tested, n_control, tables, WIN_SIZE, ordinals, rows, &error)) { fprintf(stderr, "Error: %s\n", error.c_str()); return 1; }
      const size_t cols = (size_t)(n_tested + n_control);
      for (size_t k = 0; k < ordinals.size(); k++) {
        scanners[0]->PrintIntervalAt(out_file, ordinals[k]);
        for (size_t j = 0; j < cols; j++) fprintf(out_file, "\t%d", rows[k * cols + j]);
        fprintf(out_file, "\n");
      }
    }
    fclose(out_file);
  }

  // CreateRscript (:264-284) without the script: only the existence of -R is checked
  if (strlen(RSCRIPT) > 0) {
    FILE *f = fopen(RSCRIPT, "r");
    if (f == NULL) { fprintf(stderr, "Error: R script file '%s' not found!\n", RSCRIPT); return 1; }
    fclose(f);
  }
  fprintf(stderr, "Plot step skipped: this build writes the .dat and .params files only (no R script is written or run).\n");
  GtxFinish(0);
  return 0;
}
