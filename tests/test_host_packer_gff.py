"""GFF / GTF input on the host (csrc/gtx_bed.cpp ParseGffLine, through gtx_packtool --gff, and the CLIs as far as they get without a
device): the packed reads of a GFF file are those of its BED6 restatement (tests/gff_text.py), detection follows the reference's
first-line rule, the '##' header is echoed or hidden, the reader's errors carry their text and line numbers, a '.' strand is counted
with -i and reported without, and the drivers that print query lines still refuse GFF."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import gff_cases as gc
import gff_text as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
PACK = os.path.join(BIN, "gtx_packtool")
OVERLAPS = os.path.join(BIN, "genomic_overlaps")
SCANS = os.path.join(BIN, "genomic_scans")
NAMES = ["chr1", "chr10", "chr2", "chrX"]
ENV = dict(os.environ, GTX_NO_WARMUP="1")
NO_DEVICE = "no usable HIP device"            # where a run without a GPU ends once its input has been accepted
UNSUPPORTED = "\nError: unsupported input format!\n\n"
STRAND_MSG = "GFF strand '.' is neither '+' nor '-': such a feature is counted only when the strand is ignored (-i)!"


def pack(args, path, gff):
    r = subprocess.run([PACK] + args + (["--gff"] if gff else []) + ["-c", ",".join(NAMES), str(path)], capture_output=True)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def cli(tool, args, cwd, stdin=None):
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, cwd=cwd, env=ENV, input=stdin)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gff")
    rng = np.random.default_rng(7)
    # (no header here: the packer of a BED file takes no header lines, and the line numbers of the two files must agree; a chromosome
    # outside the -c list is dropped)
    for name, kw in (("g9", dict(tokens=9)), ("g8", dict(tokens=8)), ("g10", dict(tokens=10)), ("mixed", dict(tokens=(8, 9, 10))),
                     ("num", dict(tokens=(9, 10), numeric_label=True)), ("dots", dict(tokens=9, strands="+-."))):
        text = gt.make_gff(rng, 30000, NAMES + ["chrM"], header=False, **kw)            # ~3 MB: several pieces per block
        (d / (name + ".gff")).write_text(text)
        (d / (name + ".bed")).write_text(gt.gff_file_to_bed(text, numeric_label=name == "num"))
    with gzip.open(d / "g9.gff.gz", "wb") as f:
        f.write((d / "g9.gff").read_bytes())
    (d / "r.bed").write_text("chr1\t99\t120\tr1\t0\t+\nchr1\t250\t260\tr2\t0\t-\n")
    (d / "genome.bed").write_text("".join("%s\t0\t2100000\n" % n for n in NAMES))
    return d


MODES = [["os"], ["ou"], ["os", "-s"], ["os", "-a"], ["ou", "-a", "-l", "5"], ["su"], ["ss"], ["su", "-a", "-l", "3"]]


PAIRS = [(m, n) for m in MODES for n in ("g9", "g8", "g10", "mixed", "num") if "-l" not in m or n == "num"]      # (label values: the file with numeric labels)


@pytest.mark.parametrize("mode,name", PAIRS, ids=[" ".join(m) + " " + n for m, n in PAIRS])
def test_gff_packs_like_its_bed(files, mode, name):
    """every feature is the BED6 line of the same chromosome, strand and interval [START - 1, END); numeric labels are its weights"""
    want = pack(mode, files / (name + ".bed"), False)
    got = pack(mode, files / (name + ".gff"), True)
    assert want[0] == (1 if "-s" in mode else 0), want[2]            # (-s: the file is not sorted by strand -- the same error, same line)
    assert got == want
    if name == "g9":
        assert pack(mode, files / "g9.gff.gz", True) == want
        if want[0] == 0:                                             # the leading '##' lines are skipped, whatever they say
            (files / "g9h.gff").write_text("##gff-version 2\n##chr1\tsrc\texon\t1\t2\t.\t+\t.\n" + (files / "g9.gff").read_text())
            assert pack(mode, files / "g9h.gff", True) == want


@pytest.mark.parametrize("threads", ["1", "3", "16"])
def test_thread_count_does_not_matter(files, threads):
    base = pack(["os", "-a", "-t", "1"], files / "mixed.gff", True)
    assert base[0] == 0
    assert pack(["os", "-a", "-t", threads], files / "mixed.gff", True) == base
    assert pack(["ou", "-t", threads, "-b", "5000", "-l", "4"], files / "num.gff", True) == pack(["ou", "-t", "1", "-l", "4"], files / "num.gff", True)


def test_the_dot_strand_with_and_without_the_strand(files):
    """strand '.': a feature like any other when the strand is ignored (its BED line says '.', BED's '+'); the first such line is an
    error of a strand-aware run -- also on a chromosome no reference region has"""
    for mode in (["ou"], ["os"], ["su"], ["ss"]):
        want = pack(mode, files / "dots.bed", False)
        assert want[0] == 0 and pack(mode, files / "dots.gff", True) == want
    lines = (files / "dots.gff").read_text().split("\n")
    first = next(k for k, l in enumerate(lines) if l.split("\t")[6] == ".")
    for mode in (["ou", "-a"], ["os", "-a"], ["su", "-a", "-t", "7"], ["ss", "-a", "-t", "3"]):
        rc, out, err = pack(mode, files / "dots.gff", True)
        assert (rc, err) == (1, "\nError: Line %d: %s\n" % (first + 1, STRAND_MSG)), mode


ERRORS = [
    ("seven columns", "chr1\tsrc\texon\t100\t200\t.\t+", "wrong number of tokens for GFF format!"),
    ("eleven columns", "chr1\tsrc\texon\t100\t200\t.\t+\t.\tg\tc\tmore", "wrong number of tokens for GFF format!"),
    ("three columns", "chr1\t100\t200", "wrong number of tokens for GFF format!"),
    ("comment", "#a comment", "wrong number of tokens for GFF format!"),
    ("late header", "##gff-version 3", "wrong number of tokens for GFF format!"),
    ("coordinate", "chr1\tsrc\texon\t100\t2147483646\t.\t+\t.", "coordinate does not fit the packed 32-bit representation of the MI355X path!"),
]


@pytest.mark.parametrize("name,bad,msg", ERRORS, ids=[e[0] for e in ERRORS])
def test_reader_errors(tmp_path, name, bad, msg):
    """the message after "Error: Line N: ", N counting the header, exit status 1 -- whichever piece the line falls in"""
    good = ["chr1\tsrc\texon\t%d\t%d\t.\t+\t.\tg%d" % (1000 + 10 * i, 1050 + 10 * i, i) for i in range(30000)]
    for at in (0, 17, 29000):
        if name == "late header" and at == 0:                        # (right behind the header it is one more line of it)
            continue
        lines = ["##gff-version 2", "##date x"] + good[:at] + [bad] + good[at:]
        (tmp_path / "e.gff").write_text("\n".join(lines) + "\n")
        if name != "coordinate":
            with pytest.raises(ValueError) as ex:
                gt.read_gff(bad)
            assert str(ex.value) == msg
        for mode in (["os"], ["ou", "-t", "4"], ["su", "-t", "7"]):
            rc, out, err = pack(mode, tmp_path / "e.gff", True)
            assert rc == 1
            assert err == "\nError: Line %d: %s\n" % (at + 3, msg), (mode, at)


def test_unsorted_overlap_rules_report_an_inverted_feature(tmp_path):
    (tmp_path / "i.gff").write_text("chr1\tsrc\texon\t100\t200\t.\t+\t.\nchr1\tsrc\texon\t300\t250\t.\t+\t.\nchr1\tsrc\texon\t0\t0\t.\t+\t.\n")
    assert pack(["ou"], tmp_path / "i.gff", True) == (1, "", "\nError: Line 2: start position cannot be greater than stop position!\n")
    assert pack(["su"], tmp_path / "i.gff", True) == (0, "0 100 200\n# lines=3\n", "")
    assert pack(["ss"], tmp_path / "i.gff", True)[0] == 1               # (START 0 behind START 300: not sorted)


# ---- the class layer, through the CLIs: detection, the header, errors in front of the device -----------------------------------
def _format_of(stderr):
    return [l.split("format = ")[1] for l in stderr.splitlines() if "format = " in l]


@pytest.mark.parametrize("name,line,fmt,why", gc.DETECT, ids=[d[0] for d in gc.DETECT])
def test_detection_by_the_first_line(files, name, line, fmt, why):
    """-v prints the format a set was opened with once its first line has been read; a first line its format's reader refuses says
    which reader that was; an unsupported first line ends the run there"""
    if name == "header":
        line += b"\nchr1\tsrc\texon\t100\t200\t-1.5\t+\t.\tg1"       # (a header alone is an EMPTY set; behind it even this line is GFF)
    (files / "first.txt").write_bytes(line + b"\n")
    rc, out, err = cli(OVERLAPS, ["count", "-v", "-i", "r.bed", "first.txt"], files)
    assert rc == 1 and out == ""
    if fmt is None:
        assert err.endswith(UNSUPPORTED), why
    elif fmt == "GFF":
        assert _format_of(err) == ["BED", "GFF"] and NO_DEVICE in err, (why, err)
    elif fmt == "SAM":
        assert "CIGAR" in err and "format = GFF" not in err, (why, err)
    else:
        assert "format = GFF" not in err and ("for BED format!" in err or "invalid strand" in err or _format_of(err) == ["BED", "BED"]), (why, err)


def test_header_then_a_three_column_line_is_gff(files):
    """ProcessFileHeader :3725: a '##' first line decides; the BED line behind it is a GFF line with the wrong number of tokens"""
    (files / "h3.gff").write_text("##gff-version 3\nchr1\t100\t200\n")
    rc, out, err = cli(OVERLAPS, ["count", "-v", "-i", "h3.gff", "r.bed"], files)
    assert (rc, out) == (1, "") and err.endswith("\nError: Line 2: wrong number of tokens for GFF format!\n") and "format = BED" not in err
    (files / "h0.gff").write_text("##gff-version 3\n##only a header\n")
    rc, out, err = cli(OVERLAPS, ["count", "-v", "-i", "r.bed", "h0.gff"], files)
    assert _format_of(err) == ["BED", "EMPTY"]


CALLER = os.path.join(BIN, "regions_caller")      # tests/tools/regions_caller.cpp: a set opened and walked through the class API
H_GFF = ("##gff-version 2\n##date x\n"
         'chr1\tsrc\texon\t100\t200\t.\t+\t.\tgene_id "a"; x\n'
         "  chr1\tsrc\tCDS\t150\t300\t0.5\t-\t1\tg2\ta comment\n"
         "chr2\tsrc\texon\t5\t9\t.\t.\t.\n")
H_REGIONS = ('3\tgene_id "a"; x\tchr1 + 100 200\t9 src exon . . (null)\n'
             "4\tg2\tchr1 - 150 300\t10 src CDS 0.5 1 a comment\n"
             "5\t_\tchr2 . 5 9\t8 src exon . . (null)\n")


@pytest.mark.parametrize("how", ["file", "stdin", "in-memory", "gz"])
def test_header_echo_and_hiding(files, how):
    """GenomicRegionGFF through the class API (:3501-3517: START and END as written, the strand byte raw, column 9 or "_" the label):
    the leading run of '##' lines is echoed in front of everything by a set that shows its header, and hidden by one that does not
    (:3725-3728); a '##' line further down is a data line"""
    (files / "h.gff").write_text(H_GFF)
    with gzip.open(files / "h.gff.gz", "wb") as f:
        f.write(H_GFF.encode())
    args = {"file": ["h.gff"], "stdin": [], "in-memory": ["--in-memory", "h.gff"], "gz": ["h.gff.gz"]}[how]
    stdin = H_GFF.encode() if how == "stdin" else None
    assert cli(CALLER, args, files, stdin) == (0, "format = GFF\n" + H_REGIONS, "")
    assert cli(CALLER, ["--show-header"] + args, files, stdin) == (0, "##gff-version 2\n##date x\nformat = GFF\n" + H_REGIONS, "")
    assert cli(CALLER, ["--refuse", "--show-header"] + args, files, stdin) == (1, "", UNSUPPORTED)
    (files / "h.gff").write_text(H_GFF + "##late\n")
    rc, out, err = cli(CALLER, ["--show-header", "--in-memory", "h.gff"], files)
    assert (rc, err) == (1, "\nError: Line 6: wrong number of tokens for GFF format!\n") and out == "##gff-version 2\n##date x\n"


def test_count_hides_both_headers(files):
    (files / "h.gff").write_text(H_GFF + "##late\n")
    rc, out, err = cli(OVERLAPS, ["count", "-i", "r.bed", "h.gff"], files)
    assert out == "" and NO_DEVICE in err
    rc, out, err = cli(OVERLAPS, ["count", "-i", "h.gff", "r.bed"], files)               # the reference set, in memory: line 6 is a data line
    assert (rc, out, err) == (1, "", "\nError: Line 6: wrong number of tokens for GFF format!\n")


def test_reference_set_errors_come_before_the_device(files):
    """a GFF reference file is loaded in memory: its reader's error and the strand rule are reported with their lines"""
    (files / "ref_dot.gff").write_text("##gff-version 2\nchr1\tsrc\tgene\t100\t200\t.\t+\t.\tg1\nchr1\tsrc\tgene\t300\t400\t.\t.\t.\tg2\n")
    rc, out, err = cli(OVERLAPS, ["count", "ref_dot.gff", "r.bed"], files)
    assert (rc, out, err) == (1, "", "\nError: Line 3: %s\n" % STRAND_MSG)
    for op in ("coverage", "density", "rpkm"):
        assert cli(OVERLAPS, [op, "-S", "ref_dot.gff", "r.bed"], files)[2] == "\nError: Line 3: %s\n" % STRAND_MSG
    rc, out, err = cli(OVERLAPS, ["count", "-i", "ref_dot.gff", "r.bed"], files)
    assert rc == 1 and out == "" and NO_DEVICE in err                                     # accepted: on to the device
    rc, out, err = cli(OVERLAPS, ["count", "-i", "r.bed", "dots.gff"], files)
    assert rc == 1 and out == "" and NO_DEVICE in err


def test_scanners_accept_gff_input(files):
    rc, out, err = cli(SCANS, ["counts", "-v", "-i", "-g", "genome.bed", "g9.gff"], files)
    assert rc == 1 and _format_of(err) == ["GFF"] and NO_DEVICE in err


# ---- the drivers that print lines keep refusing GFF, with today's message (no GPU needed to get there) ---------------------------
REFUSERS = [
    (OVERLAPS, ["overlap"]), (OVERLAPS, ["intersect"]), (OVERLAPS, ["offset"]), (OVERLAPS, ["overlap", "-S"]), (OVERLAPS, ["offset", "-S"]),
    (os.path.join(BIN, "genomic_subset"), []), (os.path.join(BIN, "genomic_subset"), ["-S"]),
]


@pytest.mark.parametrize("tool,argv", REFUSERS, ids=[os.path.basename(t) + " " + " ".join(a) for t, a in REFUSERS])
def test_per_pair_operations_refuse_gff(files, tool, argv):
    (files / "hdr.gff").write_text("##gff-version 2\nchr1\tsrc\texon\t100\t200\t.\t+\t.\tg1\n")
    (files / "nohdr.gff").write_text("chr1\tsrc\texon\t100\t200\t.\t+\t.\tg1\n")
    for gff in ("hdr.gff", "nohdr.gff", "g9.gff"):
        for a, b in ((gff, "r.bed"), ("r.bed", gff)):
            rc, out, err = cli(tool, argv + [a, b], files)
            assert (rc, out, err) == (1, "", UNSUPPORTED), (gff, a, b)


def test_regions_link_and_adjacent_test_refuse_gff(files):
    for tool, argv in ((os.path.join(BIN, "genomic_regions"), ["link"]), (os.path.join(BIN, "genomic_adjacent"), ["test"])):
        for gff in ("g9.gff", "g8.gff"):
            rc, out, err = cli(tool, argv + [gff], files)
            assert (rc, out) == (1, "") and err.endswith(UNSUPPORTED), (tool, gff, err)
            rc, out, err = cli(tool, argv, files, stdin=(files / gff).read_bytes())
            assert (rc, out) == (1, "") and err.endswith(UNSUPPORTED), (tool, gff, err)


# ---- genomic_peakdiff, and the genome file of the scanners and of genomic_peakdiff, take what they took -------------------------------
PEAKDIFF = os.path.join(BIN, "genomic_peakdiff")


def _tiny_gffs(files):
    (files / "hdr.gff").write_text("##gff-version 2\nchr1\tsrc\texon\t100\t200\t.\t+\t.\tg1\n")
    (files / "nohdr.gff").write_text("chr1\tsrc\texon\t100\t200\t.\t+\t.\tg1\n")
    (files / "bad2.gff").write_text("chr1\tsrc\texon\t100\t200\t.\t.\t.\tg1\nchr1\t5\t9\n")      # a '.' strand, then a line of three tokens
    return ("hdr.gff", "nohdr.gff", "bad2.gff", "g9.gff", "g8.gff")


def test_genomic_peakdiff_refuses_gff(files):
    """its read files are opened before anything else: "unsupported input format!" as before, whatever else the file holds"""
    for gff in _tiny_gffs(files):
        for args in ([gff, "r.bed"], ["r.bed," + gff, "r.bed"]):
            rc, out, err = cli(PEAKDIFF, ["-o", "pd", "-labels", "A,B", "-g", "genome.bed"] + args, files)
            if args[0].startswith("r.bed"):                           # (the second file comes behind the first one's scan: no device here)
                assert rc == 1 and out == "" and (err == UNSUPPORTED or NO_DEVICE in err), (gff, err)
            else:
                assert (rc, out, err) == (1, "", UNSUPPORTED), (gff, args, err)


def test_a_gff_genome_file_is_refused(files):
    """-g of genomic_scans counts and peaks and of genomic_peakdiff: read first, refused with the message it always had"""
    for gff in _tiny_gffs(files):
        assert cli(SCANS, ["counts", "-i", "-g", gff, "r.bed"], files) == (1, "", UNSUPPORTED), gff
        assert cli(SCANS, ["counts", "-S", "-g", gff, "g9.gff"], files) == (1, "", UNSUPPORTED), gff
        assert cli(SCANS, ["peaks", "-i", "-g", gff, "r.bed", "r.bed"], files) == (1, "", UNSUPPORTED), gff
        assert cli(PEAKDIFF, ["-o", "pd", "-labels", "A,B", "-g", gff, "r.bed", "r.bed"], files) == (1, "", UNSUPPORTED), gff
    # ... and the switch is back on behind it: the input of the same run is still read as GFF
    rc, out, err = cli(SCANS, ["counts", "-v", "-i", "-g", "genome.bed", "g9.gff"], files)
    assert rc == 1 and _format_of(err) == ["GFF"] and NO_DEVICE in err, err
