"""SAM input on the host (csrc/gtx_bed.cpp ParseSamLine, through gtx_packtool --sam): the packed reads of a SAM file are those of its
BED6 / BED12 restatement (tests/sam_text.py), the reader's errors carry the reference's text and line numbers, and the drivers that
print query lines still refuse SAM."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import sam_text as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
PACK = os.path.join(BIN, "gtx_packtool")
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["chr1", "chr10", "chr2", "chrX"]


def pack(args, path, sam):
    r = subprocess.run([PACK] + args + (["--sam"] if sam else []) + ["-c", ",".join(NAMES), str(path)], capture_output=True)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam")
    rng = np.random.default_rng(5)
    # (no header here: the packer of a BED file takes no header lines, and the line numbers of the two files must agree; a chromosome
    # outside the -c list is dropped)
    sam = st.make_sam(rng, 30000, NAMES + ["chrM"], spliced=0.15, header=False)          # ~3 MB: several pieces per block
    (d / "a.sam").write_text(sam)
    (d / "a.bed").write_text(st.sam_file_to_bed(sam))
    plain = st.make_sam(rng, 20000, NAMES + ["chrM"], numeric_qname=True, header=False)
    (d / "p.sam").write_text(plain)
    (d / "p.bed").write_text(st.sam_file_to_bed(plain))
    with gzip.open(d / "p.sam.gz", "wb") as f:
        f.write(plain.encode())
    return d


MODES = [["os"], ["ou"], ["os", "-s"], ["os", "-a"], ["ou", "-a", "-l", "5"], ["su"], ["ss"], ["su", "-a", "-l", "3"]]


@pytest.mark.parametrize("mode", MODES, ids=[" ".join(m) for m in MODES])
def test_plain_sam_packs_like_its_bed(files, mode):
    """alignments without N: every read is the BED6 line of the same chromosome, strand, label and interval"""
    want = pack(mode, files / "p.bed", False)
    got = pack(mode, files / "p.sam", True)
    assert want[0] == (1 if "-s" in mode else 0), want[2]            # (-s: the file is not sorted by strand -- the same error, same line)
    assert got == want
    assert pack(mode, files / "p.sam.gz", True) == want


@pytest.mark.parametrize("mode", [["os", "-m"], ["ou", "-m"], ["os", "-g"], ["ou", "-e"], ["ou", "-a", "-e", "-l", "4"], ["os", "-s", "-m"]])
def test_spliced_sam_packs_like_its_bed12(files, mode):
    """spliced reads are the multi-interval regions of their BED12 restatement: listed, on their envelope, or one read per interval"""
    want = pack(mode, files / "a.bed", False)
    got = pack(mode, files / "a.sam", True)
    if "-s" in mode:                                                 # (not sorted by strand: the same error at the same line)
        assert want[0] == 1 and got == want
        return
    assert want[0] == 0, want[2]
    assert got == want
    assert "# blocks" in got[1] or "-m" not in mode


def test_spliced_sam_outside_the_scanners(files):
    """a spliced read where the reduction takes none (the scanners): the BED12 error, at its line"""
    want = pack(["su"], files / "a.bed", False)
    got = pack(["su"], files / "a.sam", True)
    assert got[0] == want[0] == 1
    assert got[2] == want[2]


@pytest.mark.parametrize("threads", ["1", "3", "16"])
def test_thread_count_does_not_matter(files, threads):
    base = pack(["os", "-m", "-t", "1"], files / "a.sam", True)
    assert base[0] == 0
    assert pack(["os", "-m", "-t", threads], files / "a.sam", True) == base
    assert pack(["ou", "-t", threads, "-b", "5000"], files / "p.sam", True) == pack(["ou", "-t", "1"], files / "p.sam", True)


def _line(qname="q", flag=0, rname="chr1", pos=100, cigar="10M", seq="ACGTACGTAC", tags=""):
    qual = "*" if seq == "*" else "F" * len(seq)
    return "%s\t%s\t%s\t%s\t60\t%s\t*\t0\t0\t%s\t%s%s" % (qname, flag, rname, pos, cigar, seq, qual, tags)


def test_cigar_and_seq_forms(tmp_path):
    """'*' CIGAR with and without '*' SEQ, every accepted operation, a zero-length first interval, a header of several lines"""
    lines = ["@HD\tVN:1.6", "@SQ\tSN:chr1\tLN:9999", "@PG\tID:x",
             _line("a", 0, "chr1", 100, "*", "ACGTA"),                    # 5M
             _line("b", 16, "chr1", 120, "*", "*"),                       # 1M
             _line("c", 0, "chr1", 130, "2H3S4M1I2D2P1X2-3H", "ACGTACGTA"),
             _line("d", 16, "chr1", 150, "5N10M", "*"),                   # [150, 149] then [155, 164]
             _line("e", 0, "chr1", 170, "3M0N4M", "ACGTACG"),
             _line("f", 0, "chr1", 190, "4M10N", "ACGT"),                 # the N closes [190, 193], nothing after it
             _line("g", 0, "chr1", 200, "1M1D", "A")]
    text = "\n".join(lines) + "\n"
    (tmp_path / "f.sam").write_text(text)
    (tmp_path / "f.bed").write_text("\n".join(l for l in st.sam_file_to_bed(text).split("\n")[3:]))
    for mode in (["os", "-m"], ["ou", "-a", "-e"], ["os", "-g", "-l", "9"]):
        want = pack(mode, tmp_path / "f.bed", False)
        assert want[0] == 0, want[2]
        assert pack(mode, tmp_path / "f.sam", True) == want
    out = pack(["os", "-m", "-a"], tmp_path / "f.sam", True)[1].splitlines()
    for want in ("0 100 104", "4 120 120", "0 130 136", "0 190 193", "0 200 201"):   # (chr1 is class 0; its '-' reads class 4)
        assert want in out
    assert "# blocks 4 150 164 2 150 149 155 164" in out
    assert "# blocks 0 170 176 2 170 172 173 176" in out


ERRORS = [
    ("ten columns", "q\t0\tchr1\t100\t60\t10M\t*\t0\t0\tACGTACGTAC", "number of tokens should be at least 11 for SAM format!"),
    ("trailing tab", "q\t0\tchr1\t100\t60\t10M\t*\t0\t0\tACGTACGTAC\t", "number of tokens should be at least 11 for SAM format!"),
    ("equals op", _line(cigar="5=5M"), "unknown CIGAR operation type '='!"),
    ("unknown op", _line(cigar="5M5Q"), "unknown CIGAR operation type 'Q'!"),
    ("fragment", _line(cigar="8M", seq="ACGTACGTAC"),
     "length of aligned fragment does not match CIGAR string: \n  LABEL = q\n  CIGAR = 8M\n  length(SEQ) = 10\n"),
    ("soft clip only", _line(cigar="10S"), "SAM alignment without a reference interval (its CIGAR string has no M, D, X or N operation of positive length)!"),
    ("insertion only", _line(cigar="10I"), "SAM alignment without a reference interval (its CIGAR string has no M, D, X or N operation of positive length)!"),
]


@pytest.mark.parametrize("name,bad,msg", ERRORS, ids=[e[0] for e in ERRORS])
def test_reader_errors(tmp_path, name, bad, msg):
    """the reference's message after "Error: Line N: ", N counting the header, exit status 1 -- whichever piece the line falls in"""
    good = [_line("q%d" % i, 0, "chr1", 1000 + 10 * i) for i in range(30000)]
    for at in (0, 17, 29000):
        lines = ["@HD\tVN:1.6", "@CO\tx"] + good[:at] + [bad] + good[at:]
        (tmp_path / "e.sam").write_text("\n".join(lines) + "\n")
        with pytest.raises(ValueError) as ex:
            st.read_sam(bad)
        assert str(ex.value) == msg
        for mode in (["os"], ["ou", "-t", "4"], ["su", "-t", "7"]):
            rc, out, err = pack(mode, tmp_path / "e.sam", True)
            assert rc == 1
            assert err == "\nError: Line %d: %s\n" % (at + 3, msg), (mode, at)


def test_golden_fixture():
    """a hand-derived file: its packed reads written out by hand (tests/golden/g12_*)"""
    rc, out, err = pack(["os", "-m", "-a"], os.path.join(GOLD, "g12_reads.sam"), True)
    assert rc == 0, err
    assert out == open(os.path.join(GOLD, "g12_reads.packed")).read()
    rc, out, err = pack(["ou"], os.path.join(GOLD, "g12_bad_fragment.sam"), True)
    assert (rc, err) == (1, open(os.path.join(GOLD, "g12_bad_fragment.err")).read())


def _pack_file(src, out, sam):
    r = subprocess.run([PACK, "pack"] + (["--sam"] if sam else []) + [str(src), str(out)], capture_output=True)
    return r.returncode, r.stderr.decode()


def test_packed_region_file_from_sam(tmp_path, files):
    """gtx_packtool pack --sam: the .gtx of a SAM file (11, 12 and 13 columns) is that of its BED restatement"""
    cols = {len(l.split("\t")) for l in (files / "p.sam").read_text().splitlines()}
    assert {11, 12, 13} <= cols
    assert _pack_file(files / "p.sam", tmp_path / "x1.gtx", True) == (0, "")
    assert _pack_file(files / "p.bed", tmp_path / "x0.gtx", False) == (0, "")
    assert (tmp_path / "x1.gtx").read_bytes() == (tmp_path / "x0.gtx").read_bytes()


def test_packed_region_file_one_tag_and_spliced(tmp_path):
    """an alignment with one optional tag (12 columns) is an ordinary read; a spliced one cannot go into a packed region file"""
    one_tag = [_line("a", 0, "chr1", 100, tags="\tNM:i:0"), _line("b", 16, "chr2", 200, tags="\tNM:i:1")]
    (tmp_path / "t.sam").write_text("@HD\tVN:1.6\n" + "\n".join(one_tag) + "\n")
    (tmp_path / "t.bed").write_text("\n".join(st.to_bed(l) for l in one_tag) + "\n")
    assert _pack_file(tmp_path / "t.sam", tmp_path / "t1.gtx", True) == (0, "")
    assert _pack_file(tmp_path / "t.bed", tmp_path / "t0.gtx", False) == (0, "")
    assert (tmp_path / "t1.gtx").read_bytes() == (tmp_path / "t0.gtx").read_bytes()
    (tmp_path / "s.sam").write_text("\n".join(one_tag + [_line("c", 0, "chr2", 300, "5M10N5M")]) + "\n")
    assert _pack_file(tmp_path / "s.sam", tmp_path / "s.gtx", True) == (
        1, "\nError: Line 3: a spliced SAM alignment (a region of several intervals) cannot be kept in a packed region file!\n")


def test_cigar_ending_in_digits(tmp_path):
    """digits at the end of a CIGAR are an operation found in every set (reference and fragment length) and end it"""
    lines = [_line("a", 0, "chr1", 100, "10M5", "*"),                  # [100, 114]
             _line("b", 0, "chr1", 200, "10M5", "ACGTACGTACGTACG"),    # a fragment of 15: SEQ of 15 matches
             _line("c", 0, "chr1", 300, "5S5", "ACGTACGTAC")]          # [300, 304]
    (tmp_path / "d.sam").write_text("\n".join(lines) + "\n")
    (tmp_path / "d.bed").write_text("\n".join(st.to_bed(l) for l in lines) + "\n")
    assert pack(["ou"], tmp_path / "d.sam", True) == (0, "0 100 114\n0 200 214\n0 300 304\n# lines=3\n", "")
    assert pack(["ou"], tmp_path / "d.sam", True) == pack(["ou"], tmp_path / "d.bed", False)
    bad = _line("e", 0, "chr1", 400, "10M5", "ACGTACGTAC")
    (tmp_path / "e.sam").write_text("\n".join(lines + [bad]) + "\n")
    msg = "length of aligned fragment does not match CIGAR string: \n  LABEL = e\n  CIGAR = 10M5\n  length(SEQ) = 10\n"
    assert pack(["ou"], tmp_path / "e.sam", True) == (1, "", "\nError: Line 4: %s\n" % msg)
    with pytest.raises(ValueError) as ex:
        st.read_sam(bad)
    assert str(ex.value) == msg


# ---- the drivers that print query lines in their own format keep refusing SAM, with today's message (no GPU needed to get there)
OVERLAPS = os.path.join(BIN, "genomic_overlaps")
APPS = os.path.join(BIN, "genomic_apps")


@pytest.mark.parametrize("argv", [["overlap"], ["intersect"], ["offset"], ["overlap", "-S"], ["offset", "-S"]], ids=lambda a: " ".join(a))
def test_per_pair_operations_refuse_sam(files, argv):
    env = dict(os.environ, GTX_NO_WARMUP="1")
    for a, b in ((files / "p.sam", files / "p.bed"), (files / "p.bed", files / "p.sam")):
        r = subprocess.run([OVERLAPS] + argv + [str(a), str(b)], capture_output=True, env=env)
        assert r.returncode == 1
        assert r.stderr.decode() == "\nError: unsupported input format!\n\n"
        assert r.stdout == b""


def test_genomic_apps_refuses_sam(files):
    env = dict(os.environ, GTX_NO_WARMUP="1")
    r = subprocess.run([APPS, "profile", "-o", str(files / "out"), "-colors", "red", "-legend", "L", str(files / "p.bed"), str(files / "p.sam")],
                       capture_output=True, env=env)
    assert r.returncode == 1
    assert r.stderr.decode().endswith("Error: unsupported input format!\n\n")
