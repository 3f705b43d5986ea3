// genomic_apps -- MI355X edition of the `profile` and `heatmap` operations of GenomicTools' genomic_apps (reference driver:
// gtools/genomic_apps.cpp:95-240 options, :466-655 heatmap, :752-895 profile).  Same command line, same PREFIX.params and
// PREFIX.dat, same errors; the bins are GtxSignalBins of this package, i.e. the fused HIP pass of gtx_signal_bins (walk, 5'
// offset, bin, accumulate) through libgtx.so.
//
// The plot step is not part of this build: the reference writes an R script from templates of its own and runs `R CMD BATCH`
// on it.  Here the `-R` file must still exist (the reference's check), no PREFIX.r is written and nothing is run; one line on
// stderr says so.  `-reuse` therefore only rewrites PREFIX.params.  `peakdiff` (GSL distribution functions, quantile
// normalisation and R) is refused.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "genomic_intervals.h"
#include "gtx_cmdline.h"

static const char *PROGRAM = "genomic_apps";
static const long int BUFFER_SIZE = 10000;

// GetNextToken(&p, delim) (core.cpp:613-625): leading blanks skipped, the token runs to the delimiter or the end
static std::string NextToken(const char *&p, char delim)
{
  while (*p == ' ') p++;
  const char *e = p;
  while (*e && *e != delim) e++;
  std::string t(p, (size_t)(e - p));
  p = *e ? e + 1 : e;
  return t;
}

// CountTokens (core.cpp:577-592)
static int CountTokens(const char *s, char delim)
{
  int k = 0, n = 0;
  while (s[k] == ' ') k++;
  for (;;) {
    if (s[k] == 0) return n;
    while (s[k] != 0 && s[k] != delim) k++;
    if (s[k] == delim) k++;
    n++;
    while (s[k] == ' ') k++;
    if (s[k] == 0) return n;
  }
}

// Tokenize (genomic_apps.cpp:245-257)
static std::vector<std::string> Tokenize(const char *s, char delim)
{
  std::vector<std::string> out;
  const int n = CountTokens(s, delim);
  const char *p = s;
  for (int k = 0; k < n; k++) out.push_back(NextToken(p, delim));
  return out;
}

static FILE *OpenOut(const std::string &name)
{
  FILE *f = fopen(name.c_str(), "w");
  if (f == NULL) { fprintf(stderr, "Error: cannot open file '%s' for writing!\n", name.c_str()); exit(1); }
  return f;
}

// the command line as the last line of PREFIX.params: an argument with a blank in it quoted
static void PrintArgs(FILE *f, int argc, char *argv[])
{
  for (int i = 0; i < argc; i++)
    if (strchr(argv[i], ' ') == NULL) fprintf(f, "%s%c", argv[i], i < argc - 1 ? ' ' : '\n');
    else fprintf(f, "'%s'%c", argv[i], i < argc - 1 ? ' ' : '\n');
}

// CreateRscript (:264-284) without the script: only the existence of -R is checked
static void CheckRscript(const char *name)
{
  if (strlen(name) == 0) return;
  FILE *f = fopen(name, "r");
  if (f == NULL) { fprintf(stderr, "Error: R script file '%s' not found!\n", name); exit(1); }
  fclose(f);
}

// :521-537 / :770-785
static void BinGeometry(bool norm_ref_len, double bin_size_opt, long nbins_opt, double bin_min, double bin_max, long int *n_bins, double *bin_size)
{
  if (bin_size_opt > 0) {
    *bin_size = bin_size_opt;
    if (norm_ref_len && (*bin_size > 1.0)) { fprintf(stderr, "Error: bin size cannot be greater than 1 when --norm-ref-length is set!\n"); exit(1); }
    *n_bins = (bin_max - bin_min) / *bin_size;
  } else {
    *n_bins = nbins_opt > 0 ? nbins_opt : (norm_ref_len ? 100 : (bin_max - bin_min) / 100);
    *bin_size = nbins_opt > 0 ? (bin_max - bin_min) / *n_bins : (norm_ref_len ? (bin_max - bin_min) / 100 : 100);
  }
}

// the reference set in memory, each region's 5' interval moved upstream and its 3' interval downstream (:500-510, :816-823)
static GenomicRegionSet *LoadShifted(const std::string &file, bool verbose, long int up, long int down)
{
  GenomicRegionSet *set = new GenomicRegionSet((char *)file.c_str(), BUFFER_SIZE, verbose, true, true);
  for (long int k = 0; k < set->n_regions; k++) {
    GenomicRegion *r = set->R[k];
    GenomicInterval *r5p = r->I.front()->STRAND == '+' ? r->I.front() : r->I.back();
    GenomicInterval *r3p = r->I.front()->STRAND == '+' ? r->I.back() : r->I.front();
    // ShiftPos(start_shift, stop_shift, strand_aware = true) (genomic_intervals.cpp:524-531)
    if (r5p->STRAND == '-') r5p->STOP -= -up; else r5p->START += -up;
    if (r3p->STRAND == '-') r3p->START -= down; else r3p->STOP += down;
  }
  return set;
}

static void PlotNote() { fprintf(stderr, "Plot step skipped: this build writes the .dat and .params files only (no R script is written or run).\n"); }

int main(int argc, char *argv[])
{
  GtxAcceptSAM(false);                                        // (SAM input stays unsupported here)
  if (argc < 2) {
    fprintf(stderr, "\nUSAGE: \n  %s OPERATION [OPTIONS] INPUT-FILES\n\nOPERATIONS (MI355X path): \n"
                    "  heatmap    Create heatmap profile of signal region in reference region.\n"
                    "  profile    Create profile(s) of signal regions in reference regions.\n\n", PROGRAM);
    return 1;
  }
  const std::string op = argv[1];
  if (op == "peakdiff") { fprintf(stderr, "Operation 'peakdiff' is outside the MI355X path of this build (it needs GSL's distribution functions, quantile normalisation and R)!\n"); return 1; }
  if (op != "heatmap" && op != "profile") { fprintf(stderr, "Unknown operation '%s'!\n", op.c_str()); return 1; }
  const bool heatmap = op == "heatmap";

  bool HELP, HELP2, VERBOSE, REUSE, IGNORE_STRAND, SKIP_REF_GAPS, NORM_REF_LEN, NORM_BY_REF = false, NORM_BY_SIGNAL, NORM_BY_BIN_SIZE;
  const char *RSCRIPT, *OUT_PREFIX, *SHIFT, *LEGEND = "", *COLORS, *TITLE, *XLABEL, *YLABEL, *IMAGE_TYPE, *IMAGE_SIZE;
  double MAX_LABEL_VALUE, BIN_SIZE;
  long NBINS, NBINS_COMBINE = 1, IMAGE_RESOLUTION;
  gtxhost::Options opts;                                                    // :152-230, in the reference's order
  opts.Flag("--help", &HELP, "help");
  opts.Flag("-h", &HELP2, "help");
  opts.Flag("-v", &VERBOSE, "verbose mode");
  opts.Flag("-reuse", &REUSE, "reuse histogram data; update paramaters only");
  opts.Str("-R", &RSCRIPT, "", "R script file to use (not required)");
  opts.Str("-o", &OUT_PREFIX, "", "prefix for output files (required)");
  opts.Flag("-i", &IGNORE_STRAND, "ignore strand while finding overlaps");
  opts.Flag("--skip-ref-gaps", &SKIP_REF_GAPS, "ignore gaps in reference regions when computing offsets");
  opts.Double("--max-label-value", &MAX_LABEL_VALUE, 1.0, "maximum query region label value to be used");
  opts.Flag("--norm-ref-length", &NORM_REF_LEN, "normalize reference region length to 1.0");
  if (!heatmap) opts.Flag("--norm-by-ref-regions", &NORM_BY_REF, "normalize by the number of reference regions");
  opts.Flag("--norm-by-total-reads", &NORM_BY_SIGNAL, "normalize by the total number of reads");
  opts.Flag("--norm-by-bin-size", &NORM_BY_BIN_SIZE, "normalize by the bin size");
  opts.Double("--bin-size", &BIN_SIZE, 0, "bin size; overrides -nbins (0 = auto)");
  opts.Long("-nbins", &NBINS, 0, "number of bins (0 = auto)");
  if (heatmap) opts.Long("--nbins-smooth", &NBINS_COMBINE, 1, "number of bins to combine for smoothing effect");
  opts.Str("-shift", &SHIFT, "5000,5000", "comma-separated upstream/downstream distances from reference center");
  if (heatmap) opts.Str("-colors", &COLORS, "", "comma-separated colors for heatmap pixels");
  else {
    opts.Str("-legend", &LEGEND, "", "comma-separated legend labels for line plot");
    opts.Str("-colors", &COLORS, "", "comma-separated colors for line plot");
  }
  opts.Str("-title", &TITLE, "", heatmap ? "heatmap comma-separated titles" : "plot title");
  opts.Str("-xlab", &XLABEL, "", heatmap ? "heatmap x-axis label" : "plot x-axis label");
  opts.Str("-ylab", &YLABEL, "", heatmap ? "heatmap y-axis label" : "plot y-axis label");
  opts.Str("-itype", &IMAGE_TYPE, "pdf", "image format type {pdf,tif}");
  opts.Str("-isize", &IMAGE_SIZE, heatmap ? "2000,4000" : "2000,2000", "comma-separated image dimensions (for tif format only)");
  opts.Long("-ires", &IMAGE_RESOLUTION, heatmap ? 600 : 300, "image resolution in dpi (for tif format only)");
  const int next_arg = opts.Parse(argc, argv, 2);
  if (HELP || HELP2 || argc - next_arg < 2) {
    opts.Usage(PROGRAM, op.c_str(), heatmap ? "[OPTIONS] COMMA-SEPARATED-SIGNAL-REG-FILES REFERENCE-REG-FILE"
                                            : "[OPTIONS] COMMA-SEPARATED-SIGNAL-REG-FILES COMMA-SEPARATED-REFERENCE-REG-FILES");
    return 1;
  }
  if (strcmp(IMAGE_TYPE, "pdf") != 0 && strcmp(IMAGE_TYPE, "tif") != 0) { fprintf(stderr, "Error: unsupported image format '%s'!\n", IMAGE_TYPE); return 1; }
  _MESSAGES_ = VERBOSE;
  if (strlen(OUT_PREFIX) == 0) { fprintf(stderr, "Error: prefix for output files must be specified using the -o option!\n"); return 1; }

  const std::vector<std::string> signal_file = Tokenize(argv[next_arg], ','), ref_file = Tokenize(argv[next_arg + 1], ',');
  const int n_signal_files = (int)signal_file.size(), n_ref_files = (int)ref_file.size();
  const std::string data_file_name = std::string(OUT_PREFIX) + ".dat", param_file_name = std::string(OUT_PREFIX) + ".params";
  const int imres = (int)IMAGE_RESOLUTION, nbins_opt = (int)NBINS, nbins_combine = (int)NBINS_COMBINE;

  if (heatmap) {                                                            // :466-655
    const char *shift = SHIFT;
    const long int shift_upstream = atol(NextToken(shift, ',').c_str());
    const long int shift_downstream = atol(NextToken(shift, ',').c_str());
    if (n_ref_files > 1) { fprintf(stderr, "Error: only one reference file allowed!\n"); return 1; }
    if (CountTokens(COLORS, ',') != n_signal_files) { fprintf(stderr, "Error: number of colors must match number of signal files!\n"); return 1; }
    if (CountTokens(TITLE, ',') != n_signal_files) { fprintf(stderr, "Error: number of titles must match number of signal files!\n"); return 1; }
    FILE *param_file = OpenOut(param_file_name);
    fprintf(param_file, "%ld\n%ld\n%s\n%s\n%s\n%s\n%s\n%d\n%d\n", shift_upstream, shift_downstream, COLORS, TITLE, XLABEL, YLABEL, IMAGE_SIZE, imres, n_signal_files);
    PrintArgs(param_file, argc, argv);
    fclose(param_file);
    CheckRscript(RSCRIPT);
    if (!REUSE) {
      const double bin_min = NORM_REF_LEN ? 0.0 : -shift_upstream, bin_max = NORM_REF_LEN ? 1.0 : shift_downstream;
      long int n_bins; double bin_size;
      BinGeometry(NORM_REF_LEN, BIN_SIZE, nbins_opt, bin_min, bin_max, &n_bins, &bin_size);
      if (nbins_combine >= n_bins) { fprintf(stderr, "Error: number of bins to combine cannot be greater than total number of bins!\n"); return 1; }
      if (VERBOSE) {
        fprintf(stderr, "Bin parameters:\n* bin min = %f\n* bin max = %f\n* bin size = %f\n* number of bins = %ld\n* number of bins for smoothing = %d\n",
                bin_min, bin_max, bin_size, n_bins, nbins_combine);
      }
      GenomicRegionSet *RefRegSet = LoadShifted(ref_file[0], VERBOSE, shift_upstream, shift_downstream);
      const long int n_ref = RefRegSet->n_regions;
      std::vector<std::vector<double> > bins((size_t)n_signal_files);
      std::vector<unsigned long int> n_signal_reg((size_t)n_signal_files, 0);
      const GtxSignalSpec spec{IGNORE_STRAND, SKIP_REF_GAPS, NORM_REF_LEN, true, bin_min, bin_max, MAX_LABEL_VALUE, n_bins};
      for (int n = 0; n < n_signal_files; n++) {
        if (VERBOSE) fprintf(stderr, "Creating heatmap of '%s' in '%s'...\n", signal_file[n].c_str(), ref_file[0].c_str());
        GenomicRegionSet TestRegSet((char *)signal_file[n].c_str(), BUFFER_SIZE, VERBOSE, false, true);
        UnsortedGenomicRegionSetOverlaps Overlaps(&TestRegSet, RefRegSet, "17,20,23,26");
        n_signal_reg[n] = GtxSignalBins(&Overlaps, spec, bins[n]);
      }
      FILE *data_file = OpenOut(data_file_name);
      fprintf(data_file, "reference-label");
      const char *titles = TITLE;
      while (titles[0] != 0) {
        const std::string t = NextToken(titles, ',');
        for (int k = 0; k < n_bins; k++) fprintf(data_file, "\t%s:bin=%d", t.c_str(), k + 1);
      }
      fprintf(data_file, "\n");
      // row = the region's ordinal (the reference indexes by ireg->n_line - n_ref1, the same while no non-region line follows the
      // first region, and out of bounds otherwise)
      auto at = [&](int s, long int r, long int q) { return q >= 0 && q < n_bins ? bins[s][(size_t)r * n_bins + q] : 0.0; };
      for (long int r = 0; r < n_ref; r++) {
        fprintf(data_file, "%s\t", RefRegSet->R[r]->LABEL);
        for (int s = 0; s < n_signal_files; s++) {
          double norm = 1.0;
          if (NORM_BY_SIGNAL) norm *= n_signal_reg[s];
          if (NORM_BY_BIN_SIZE) norm *= bin_size;
          double val = 0;
          for (int q = 0; q < nbins_combine - 1; q++) val += at(s, r, q);
          for (long int q = 0, qq = nbins_combine - 1; qq < n_bins; q++, qq++) {
            val += at(s, r, qq);
            fprintf(data_file, "%.6e%s", val / norm, qq != n_bins - 1 ? "\t" : "");
            val -= at(s, r, q);
          }
          fprintf(data_file, "%c", s != n_signal_files - 1 ? '\t' : '\n');
        }
      }
      fclose(data_file);
    }
    PlotNote();
    GtxFinish(0);
    return 0;
  }

  // profile (:752-895)
  const char *shift = SHIFT;
  const double shift_upstream = atof(NextToken(shift, ',').c_str());
  const double shift_downstream = atof(NextToken(shift, ',').c_str());
  if (CountTokens(COLORS, ',') != n_signal_files * n_ref_files) { fprintf(stderr, "Error: number of colors must match total number of lines in the plot!\n"); return 1; }
  if (CountTokens(LEGEND, ',') != n_signal_files * n_ref_files) { fprintf(stderr, "Error: number of legend labels must match total number of lines in the plot!\n"); return 1; }
  const double bin_min = NORM_REF_LEN ? 0.0 : -shift_upstream, bin_max = NORM_REF_LEN ? 1.0 : shift_downstream;
  long int n_bins; double bin_size;
  BinGeometry(NORM_REF_LEN, BIN_SIZE, nbins_opt, bin_min, bin_max, &n_bins, &bin_size);
  if (VERBOSE) fprintf(stderr, "* bin min = %f\n* bin max = %f\n* bin size = %f\n* number of bins = %ld\n", bin_min, bin_max, bin_size, n_bins);
  FILE *param_file = OpenOut(param_file_name);
  fprintf(param_file, "%f\n%f\n%s\n%s\n%s\n%s\n%s\n%s\n%d\n", bin_min, bin_max, LEGEND, COLORS, TITLE, XLABEL, YLABEL, IMAGE_SIZE, imres);
  PrintArgs(param_file, argc, argv);
  fclose(param_file);
  CheckRscript(RSCRIPT);
  if (!REUSE) {
    FILE *data_file = OpenOut(data_file_name);
    const GtxSignalSpec spec{IGNORE_STRAND, SKIP_REF_GAPS, NORM_REF_LEN, false, bin_min, bin_max, MAX_LABEL_VALUE, n_bins};
    for (int m = 0; m < n_ref_files; m++) {
      // the double shifts truncated to long at the ShiftPos call (-shift_upstream * ref_len, ref_len = 1)
      GenomicRegionSet *RefRegSet = LoadShifted(ref_file[m], VERBOSE, (long int)shift_upstream, (long int)shift_downstream);
      for (int n = 0; n < n_signal_files; n++) {
        if (VERBOSE) fprintf(stderr, "Creating profile of '%s' in '%s'...\n", signal_file[n].c_str(), ref_file[m].c_str());
        GenomicRegionSet TestRegSet((char *)signal_file[n].c_str(), BUFFER_SIZE, VERBOSE, false, true);
        UnsortedGenomicRegionSetOverlaps Overlaps(&TestRegSet, RefRegSet, "17,20,23,26");
        std::vector<double> bins;
        const unsigned long int n_signal_reg = GtxSignalBins(&Overlaps, spec, bins);
        fprintf(data_file, "%s in %s\t", signal_file[n].c_str(), ref_file[m].c_str());
        double norm = 1.0;
        if (NORM_BY_REF) norm *= RefRegSet->n_regions;
        if (NORM_BY_SIGNAL) norm *= n_signal_reg;
        if (NORM_BY_BIN_SIZE) norm *= bin_size;
        for (long int b = 0; b < n_bins; b++) fprintf(data_file, "%.6e%c", (double)bins[b] / norm, b != n_bins - 1 ? '\t' : '\n');
      }
    }
    fclose(data_file);
  }
  PlotNote();
  GtxFinish(0);
  return 0;
}
