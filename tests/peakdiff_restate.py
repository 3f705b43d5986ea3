"""The data pass of `genomic_apps peakdiff` restated in Python -- TEST INFRASTRUCTURE ONLY: the yardstick of the peakdiff tests.

ScanReadFiles (gtools/genomic_apps.cpp:314-431) as it stands there:
  * bounds = ReadBounds(genome file); effective genome size = the sum of the chromosome lengths (:320-321);
  * per read file p = CountGenomicRegions(file, false) / effective genome size (:329): every region of the file counts 1, whatever
    its label and whether or not its chromosome has bounds;
  * every file goes through an UnsortedGenomicRegionSetScanner with preprocess 'c' (:332): oracle/orc.py's scan, the windows in the
    scanners' iteration order (chromosomes as strcmp orders them, '+' block then '-' block; one block per chromosome under -i);
  * the scanners are stepped together, each value clamped to the window size (:386-389);
  * a window is kept when gsl_cdf_binomial_Q(k, p, W) <= cutoff for any sample file (:393-403): p is the file's background, or with
    controls max(background, min(control count / W, 1.0)); the tail is the oracle's orc_binomial_Q, evaluated per window, no table;
  * a kept window prints "chr strand start stop" and every file's clamped count behind tabs: sample 1, sample 2, then the controls
    (:405-412), under the header of :377-382.
params_text is PREFIX.params (:702-719).  BED parsing is oracle/restate.py's.
"""
import ctypes

import numpy as np

from oracle import orc, restate


def _binomial_q():
    L = orc.lib()
    L.orc_binomial_Q.restype = ctypes.c_double
    L.orc_binomial_Q.argtypes = [ctypes.c_long, ctypes.c_double, ctypes.c_long]
    return L.orc_binomial_Q


def is_header(line):
    return line.startswith("browser ") or line.startswith("track ")


def read_bounds(genome_lines):
    """[(chromosome, length)] as the scanners walk them: std::map order, i.e. bytes order"""
    b = {}
    for line in genome_lines:
        if line and not is_header(line):
            r = restate.parse(line)
            b.setdefault(r["chrom"], r["iv"][0][1])
    return sorted(b.items(), key=lambda kv: kv[0].encode())


def label_value(label, max_label_value):
    """GenomicRegion::GetLabelValue (genomic_intervals.cpp:1081-1085); atol of a label that is no number is 0"""
    if max_label_value <= 1:
        return 1
    try:
        v = int(label)
    except ValueError:
        v = 0
    return min(max_label_value, v)


def scan_file(lines, bounds, win_size, win_dist, ignore_strand, max_label_value):
    """(window sums in iteration order, number of regions in the file)"""
    index = {name: i for i, (name, _) in enumerate(bounds)}
    ns = 1 if ignore_strand else 2
    tri, w, n_regions = [], [], 0
    for line in lines:
        if not line or is_header(line):
            continue
        r = restate.parse(line)
        n_regions += 1
        if r["chrom"] not in index:
            continue
        cls = index[r["chrom"]] * ns + (1 if (r["minus"] and not ignore_strand) else 0)
        for s, e in r["iv"]:
            tri.append((cls, s, e)); w.append(label_value(r["label"], max_label_value))
    class_len = [ln for _, ln in bounds for _ in range(ns)]
    reads = np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    weights = np.asarray(w, dtype=np.int32) if max_label_value > 1 else None
    win, off = orc.scan(reads, class_len, win_dist, win_size, preprocess="c", weights=weights)
    return win, off, n_regions


def intervals(bounds, win_size, win_dist, ignore_strand):
    """"chr strand start stop" of every window, in iteration order"""
    out = []
    comb = win_size // win_dist
    for name, ln in bounds:
        n = ln // win_dist
        nw = 0 if n < comb else n - comb + 1
        for strand in ("+",) if ignore_strand else ("+", "-"):
            out += ["%s %s %d %d" % (name, strand, win_dist * j + 1, win_dist * j + win_size) for j in range(nw)]
    return out


class BackgroundAboveOne(Exception):
    pass


def peakdiff_dat(genome_lines, signal, ref, signal_control, ref_control, labels, win_size=500, win_dist=100, pval=1e-5, ignore_strand=False,
                 max_label_value=1):
    """(text of PREFIX.dat, number of windows, number kept); signal / ref / *_control: lists of files, a file a list of lines"""
    Q = _binomial_q()
    bounds = read_bounds(genome_lines)
    genome = sum(ln for _, ln in bounds)
    tested, controls = list(signal) + list(ref), list(signal_control) + list(ref_control)
    vec, p = [], []
    for f in tested + controls:
        win, _, n_regions = scan_file(f, bounds, win_size, win_dist, ignore_strand, max_label_value)
        vec.append(np.minimum(win, np.uint64(win_size)).astype(np.int64))
        p.append(n_regions / genome)
        if not p[-1] <= 1.0:
            raise BackgroundAboveOne()
    head = ["locus"] + ["%s count %d" % (labels[0], s + 1) for s in range(len(signal))] + ["%s count %d" % (labels[1], r + 1) for r in range(len(ref))]
    head += ["%s control count %d" % (labels[0], s + 1) for s in range(len(signal_control))]
    head += ["%s control count %d" % (labels[1], r + 1) for r in range(len(ref_control))]
    out = ["\t".join(head) + "\n"]
    where = intervals(bounds, win_size, win_dist, ignore_strand)
    assert all(len(v) == len(where) for v in vec)
    nt, kept = len(tested), 0
    for j in range(len(where)):
        keep = False
        for f in range(nt):
            k = int(vec[f][j])
            pf = max(p[f], min(float(vec[nt + f][j]) / win_size, 1.0)) if controls else p[f]
            if Q(k, pf, win_size) <= pval:
                keep = True
                break
        if keep:
            kept += 1
            out.append(where[j] + "".join("\t%d" % int(v[j]) for v in vec) + "\n")
    return "".join(out), len(where), kept


def params_text(argv, n_signal, n_ref, win_size=500, pval=1e-5, scale="winsize", norm="normq", pseudo=1.0, outliers=0.01, fdr=0.05, fold=1.0,
                fdr_bins=1, labels="", isize="3000,2000", ires=300):
    """PREFIX.params (genomic_apps.cpp:702-719); argv: the whole command line, program name first"""
    t = "n_signal %d\nn_ref %d\nwin %d\npval %.6e\nscale %s\nnorm %s\npseudo %.6e\noutliers %.6e\nfdr %.6e\nfold %.6e\nfdr_bins %d\nlabels %s\nisize %s\nires %d\n" % (
        n_signal, n_ref, win_size, pval, scale, norm, pseudo, outliers, fdr, fold, fdr_bins, labels, isize, ires)
    return t + "# " + " ".join(a if " " not in a else "'%s'" % a for a in argv) + "\n"


def case_options(options):
    """the keyword arguments of peakdiff_dat from a manifest vector's option list"""
    kw, k = {}, 0
    while k < len(options):
        o = options[k]
        if o == "-i":
            kw["ignore_strand"] = True; k += 1; continue
        v = options[k + 1]
        if o == "-w":
            kw["win_size"] = int(v)
        elif o == "-d":
            kw["win_dist"] = int(v)
        elif o == "-pval":
            kw["pval"] = float(v)
        elif o == "--max-label-value":
            kw["max_label_value"] = int(v)
        else:
            raise ValueError(o)
        k += 2
    return kw
