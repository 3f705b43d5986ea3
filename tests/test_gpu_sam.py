"""SAM alignments as the reads of genomic_overlaps count | rpkm | coverage | density and genomic_scans counts | peaks: the product on a
SAM file prints what the oracle CLI prints on its BED6 / BED12 restatement (tests/sam_text.py), with the text tokenised on the device
(GTX_TEXT_SAM, csrc/gtx_text.hip) and without; one odd line sends exactly its block back to the host packer."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import sam_text as st
from oracle import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")
TOOLS = {"overlaps": os.path.join(BIN, "genomic_overlaps"), "scans": os.path.join(BIN, "genomic_scans")}
NAMES = ["chr1", "chr10", "chr2", "chrX"]
HEADER = 1 + len(NAMES) + 1                  # @HD, @SQ per chromosome (and chrM), as make_sam writes them
ODD_AT = 50_000                              # index of the odd alignment


def run(tool, args, cwd, on_device, stdin=None):
    env = dict(os.environ, GTX_TEXT_ON_DEVICE="1" if on_device else "0", GTX_TEXT_TRACE="1", GTX_PACK_BLOCK_MB="1")
    r = subprocess.run([TOOLS[tool]] + list(args), capture_output=True, cwd=cwd, env=env, input=stdin)
    lines = r.stderr.decode().split("\n")
    trace = [l for l in lines if l.startswith("[gtx text]")]
    err = "\n".join(l for l in lines if not l.startswith("[gtx text]"))
    nums = [int(x) for x in re.findall(r": (\d+)", trace[0])] if trace else None
    return r.returncode, r.stdout.decode(), err, nums


def oracle(args, cwd):
    r = subprocess.run([orc.CLI] + list(args), capture_output=True, cwd=cwd)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def _write_pair(d, name, sam):
    (d / (name + ".sam")).write_text(sam)
    (d / (name + ".bed")).write_text(st.sam_file_to_bed(sam))


def _by_strand(sam):
    head = [l for l in sam.splitlines() if l.startswith("@")]
    body = [l.split("\t") for l in sam.splitlines() if not l.startswith("@")]
    body.sort(key=lambda t: (t[2], "-" if int(t[1]) & 16 else "+", int(t[3])))
    return "\n".join(head + ["\t".join(t) for t in body]) + "\n"


@pytest.fixture(scope="module")
def sams(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_gpu")
    rng = np.random.default_rng(101)
    refs = []
    c = rng.integers(0, len(NAMES), 3000); s = rng.integers(1000, 2_000_000, 3000); ln = rng.integers(20, 3000, 3000)
    for i in np.lexsort((s, np.array([NAMES[k] for k in c]))):
        refs.append((NAMES[c[i]], int(s[i]), int(s[i] + ln[i]), "g%d" % i, "+-"[int(rng.integers(0, 2))]))
    (d / "refs.bed").write_text("".join("%s\t%d\t%d\t%s\t0\t%s\n" % r for r in refs))
    rs = sorted(refs, key=lambda r: (r[0], r[4], r[1]))
    (d / "refs_by_strand.bed").write_text("".join("%s\t%d\t%d\t%s\t0\t%s\n" % r for r in rs))
    gen = NAMES + ["chrM"]                                                              # (a chromosome no reference region has: dropped)
    plain = st.make_sam(rng, 120_000, gen, numeric_qname=True)
    _write_pair(d, "plain", plain)
    _write_pair(d, "plain_by_strand", _by_strand(plain))
    _write_pair(d, "spliced", st.make_sam(rng, 60_000, gen, spliced=0.02))
    lines = plain.split("\n")
    at = HEADER + ODD_AT
    t = lines[at].split("\t")

    def variant(name, line, bed=True):
        v = list(lines); v[at] = line
        text = "\n".join(v)
        (d / (name + ".sam")).write_text(text)
        if bed:
            (d / (name + ".bed")).write_text(st.sam_file_to_bed(text))
    variant("odd_spliced", "\t".join(t[:5] + ["10M50N10M"] + t[6:9] + ["*", "*"]))
    variant("odd_crlf", lines[at] + "\r")
    variant("odd_equals", "\t".join(t[:5] + ["5=5M"] + t[6:9] + ["*", "*"]), bed=False)
    variant("odd_unsorted", "\t".join(t[:3] + ["1"] + t[4:]))
    variant("odd_blank", "\t".join(t[:3] + [" " + t[3]] + t[4:]))
    # reads of 1 kb (lines of ~2 KB): 128 of them are more text than a parse block stages (72 KiB) -- their blocks go to the host packer
    _write_pair(d, "long", st.make_sam(rng, 6_000, gen, read_len=1000, star_seq=0.0, star_cigar=0.0))
    v = list(lines)
    for k in range(at, at + 300):                                                       # a run of 300 such lines inside the plain file
        u = v[k].split("\t")
        v[k] = "\t".join(u[:5] + ["1000M"] + u[6:9] + ["A" * 1000, "I" * 1000] + u[11:])
    (d / "long_run.sam").write_text("\n".join(v))
    (d / "long_run.bed").write_text(st.sam_file_to_bed("\n".join(v)))
    with gzip.open(d / "plain.sam.gz", "wb") as f:
        f.write(plain.encode())
    with open(d / "genome.bed", "w") as f:
        for n in NAMES:
            f.write("%s\t0\t%d\n" % (n, 2_100_000))
    # peaks: a signal with clusters over a background, and a control
    bg = st.make_sam(rng, 40_000, NAMES, read_len=50, header=False).splitlines()
    extra = []
    for k in range(40):
        nm, p0 = NAMES[k % 4], int(rng.integers(10_000, 2_000_000))
        for j in range(40):
            extra.append("c%d\t%d\t%s\t%d\t60\t50M\t*\t0\t0\t*\t*" % (k, 16 * (j & 1), nm, p0 + int(rng.integers(0, 400))))
    sig = sorted(bg + extra, key=lambda l: (l.split("\t")[2], int(l.split("\t")[3])))
    _write_pair(d, "signal", "\n".join(sig) + "\n")
    _write_pair(d, "control", st.make_sam(rng, 40_000, NAMES, read_len=50, header=False))
    return d


RUNS = [["count", "-S", "-i"], ["count", "-i"], ["count", "-S"], ["count"], ["count", "-S", "-s"],
        ["count", "-S", "-i", "--max-label-value", "5"], ["count", "-i", "--max-label-value", "3"], ["count", "-S", "-i", "-gaps"],
        ["rpkm", "-S", "-i"], ["coverage", "-S", "-i"], ["coverage", "-i", "--max-label-value", "4"], ["density", "-S"], ["density", "-i", "-gaps"]]


def _files(mode, reads):
    if "-s" in mode:
        return ["refs_by_strand.bed", reads + "_by_strand"]
    return ["refs.bed", reads]


@pytest.mark.parametrize("on_device", [1, 0], ids=["device", "host"])
@pytest.mark.parametrize("mode", RUNS, ids=[" ".join(m) for m in RUNS])
def test_plain_sam_equals_oracle_on_its_bed(sams, mode, on_device):
    """alignments without N: every block tokenised on the device (GTX_TEXT_ON_DEVICE=1), none comes back; or all of it on the host"""
    ref, reads = _files(mode, "plain")
    want = oracle(mode + [ref, reads + ".bed"], sams)
    rc, out, err, nums = run("overlaps", mode + [ref, reads + ".sam"], sams, on_device)
    assert want[0] == 0, want[2]
    assert (rc, out) == want[:2], err
    if on_device:
        assert nums is not None and nums[0] >= 10 and nums[1] == 0 and nums[2] == 0, nums
    else:
        assert nums is None


@pytest.mark.parametrize("on_device", [1, 0], ids=["device", "host"])
@pytest.mark.parametrize("mode", [["count", "-S", "-i"], ["count", "-i", "-gaps"], ["coverage", "-S", "-i"], ["density", "-S"], ["rpkm", "-i"]],
                         ids=lambda m: " ".join(m))
def test_spliced_sam_equals_oracle_on_its_bed12(sams, mode, on_device):
    """spliced reads are multi-interval regions: the blocks that hold one come back and are counted like BED12 lines"""
    want = oracle(mode + ["refs.bed", "spliced.bed"], sams)
    rc, out, err, nums = run("overlaps", mode + ["refs.bed", "spliced.sam"], sams, on_device)
    assert want[0] == 0, want[2]
    assert (rc, out) == want[:2], err
    if on_device:
        assert nums is not None and nums[1] >= 1, nums


@pytest.mark.parametrize("name", ["odd_spliced", "odd_crlf", "odd_unsorted", "odd_blank"])
def test_one_odd_line_sends_exactly_its_block_back(sams, name):
    for mode in (["count", "-S", "-i"], ["count", "-i"], ["coverage", "-S", "-i"]):
        want = oracle(mode + ["refs.bed", name + ".bed"], sams)
        rc, out, err, nums = run("overlaps", mode + ["refs.bed", name + ".sam"], sams, True)
        assert (rc, out) == want[:2], (mode, err, want[2])
        if want[0] != 0:
            assert err.strip() == want[2].strip(), mode
        elif name == "odd_unsorted":
            assert nums is not None and nums[1] == 0, (mode, nums)      # (out of order is plain where nothing checks the order)
        else:
            assert nums is not None and nums[1] == 1, (mode, nums)


@pytest.mark.parametrize("mode", [["count", "-S", "-i"], ["coverage", "-i"], ["count", "-S", "-s"]], ids=lambda m: " ".join(m))
def test_lines_longer_than_the_staging_go_to_the_host(sams, mode):
    """128 alignments of 1 kb are more than the 72 KiB a SAM parse block stages: every block of such a file comes back, a run of
    them inside a file of short reads sends back only the block(s) it lies in -- the output is the oracle's either way"""
    for name in ("long", "long_run"):
        reads = name
        if "-s" in mode:
            (sams / (name + "_by_strand.sam")).write_text(_by_strand((sams / (name + ".sam")).read_text()))
            (sams / (name + "_by_strand.bed")).write_text(st.sam_file_to_bed((sams / (name + "_by_strand.sam")).read_text()))
        ref, reads = _files(mode, name)
        want = oracle(mode + [ref, reads + ".bed"], sams)
        rc, out, err, nums = run("overlaps", mode + [ref, reads + ".sam"], sams, True)
        assert want[0] == 0, want[2]
        assert (rc, out) == want[:2], (name, err)
        assert nums is not None, err
        if name == "long":
            assert nums[0] == 0 and nums[1] >= 5, nums
        elif "-s" not in mode:                                          # (regrouped by strand the run is spread over the file)
            assert nums[0] >= 10 and 1 <= nums[1] <= 2, nums


def test_equals_in_a_cigar_is_the_reference_error(sams):
    msg = "Error: Line %d: unknown CIGAR operation type '='!" % (HEADER + ODD_AT + 1)
    for on_device in (1, 0):
        for mode in (["count", "-S", "-i"], ["coverage", "-i"], ["rpkm", "-S"]):
            rc, out, err, nums = run("overlaps", mode + ["refs.bed", "odd_equals.sam"], sams, on_device)
            assert (rc, out, err.strip()) == (1, "", msg), (mode, on_device)


def test_stdin_and_gz(sams):
    want = oracle(["count", "-S", "-i", "refs.bed", "plain.bed"], sams)
    data = (sams / "plain.sam").read_bytes()
    for on_device in (1, 0):
        rc, out, err, nums = run("overlaps", ["count", "-S", "-i", "refs.bed"], sams, on_device, stdin=data)
        assert (rc, out) == want[:2], err
        rc, out, err, nums = run("overlaps", ["count", "-S", "-i", "refs.bed", "plain.sam.gz"], sams, on_device)
        assert (rc, out) == want[:2], err
    rc, out, err, nums = run("overlaps", ["count", "-S", "-i", "refs.bed"], sams, True, stdin=data)
    assert nums is not None and nums[0] >= 10 and nums[1] == 0, nums


def test_sam_reference_file(sams):
    """a SAM file as the reference regions: its labels are the QNAMEs, its spliced alignments multi-interval regions"""
    for mode in (["count", "-i"], ["count", "-S", "-i"], ["coverage", "-i"], ["density", "-gaps"]):
        want = oracle(mode + ["spliced.bed", "plain.bed"], sams)
        rc, out, err, nums = run("overlaps", mode + ["spliced.sam", "plain.sam"], sams, True)
        assert (rc, out) == want[:2], (mode, err)


def test_ngpu_rehearsed(sams):
    env_extra = {"GTX_GROUP_REHEARSE": "1"}
    want = oracle(["count", "-S", "-i", "refs.bed", "plain.bed"], sams)
    env = dict(os.environ, GTX_TEXT_ON_DEVICE="1", GTX_PACK_BLOCK_MB="1", **env_extra)
    r = subprocess.run([TOOLS["overlaps"], "count", "--ngpu", "2", "-S", "-i", "refs.bed", "plain.sam"], capture_output=True, cwd=sams, env=env)
    assert (r.returncode, r.stdout.decode()) == want[:2], r.stderr.decode()


SCANS = [["counts", "-i", "-g", "genome.bed", "-w", "1000", "-d", "1000", "-min", "1"],
         ["counts", "-S", "-i", "-g", "genome.bed", "-w", "500", "-d", "100", "-min", "2"],
         ["counts", "-g", "genome.bed", "-w", "1000", "-d", "500", "-min", "2"],
         ["counts", "-i", "--max-label-value", "5", "-g", "genome.bed", "-w", "2000", "-d", "1000", "-min", "1"]]


@pytest.mark.parametrize("on_device", [1, 0], ids=["device", "host"])
@pytest.mark.parametrize("args", SCANS, ids=[" ".join(a) for a in SCANS])
def test_scans_counts(sams, args, on_device):
    want = oracle(args + ["plain.bed"], sams)
    rc, out, err, nums = run("scans", args + ["plain.sam"], sams, on_device)
    assert want[0] == 0, want[2]
    assert (rc, out) == want[:2], err
    if on_device:
        assert nums is not None and nums[1] == 0, nums


@pytest.mark.parametrize("on_device", [1, 0], ids=["device", "host"])
@pytest.mark.parametrize("args", [["peaks", "-i", "-g", "genome.bed"], ["peaks", "-S", "-i", "-g", "genome.bed", "-M", "poisson"]], ids=lambda a: " ".join(a))
def test_scans_peaks(sams, args, on_device):
    want = oracle(args + ["signal.bed", "control.bed"], sams)
    rc, out, err, nums = run("scans", args + ["signal.sam", "control.sam"], sams, on_device)
    assert want[0] == 0, want[2]
    assert (rc, out) == want[:2], (err, want[2], nums)
    assert err.strip().replace(".sam", ".bed") == want[2].strip()                 # (the report lines name the input files)
    assert len(out.splitlines()) >= 5


def test_peaks_read_total_with_a_short_last_group_bed(sams):
    """BED text on the device: a block whose last 128-line group ends inside its second wave still sums the label values of all its
    lines (peaks' read totals and the p-values that follow from them)"""
    lines = (sams / "signal.bed").read_text().splitlines()
    for n in (len(lines) - 37, len(lines) - 100, len(lines) - 64):
        (sams / "short.bed").write_text("\n".join(lines[:n]) + "\n")
        args = ["peaks", "-i", "-g", "genome.bed", "short.bed", "control.bed"]
        want = oracle(args, sams)
        rc, out, err, nums = run("scans", args, sams, True)
        assert (rc, out, err.strip()) == (want[0], want[1], want[2].strip()), n


def test_c_abi_count_add_text_sam(engine, sams):
    """gtx_count_add_text(..., GTX_TEXT_SAM) on a block of plain alignments: needs_host == 0, the hits of gtx_count on its triples"""
    import gtx
    refs = []
    for l in (sams / "refs.bed").read_text().splitlines():
        t = l.split("\t")
        refs.append((NAMES.index(t[0]), int(t[1]) + 1, int(t[2])))
    engine.set_refs(np.array(refs, dtype=np.int32), len(NAMES))
    body = [l for l in (sams / "plain.sam").read_text().splitlines() if not l.startswith("@")][:20000]
    tri = []
    for l in body:
        chrom, strand, label, iv = st.read_sam(l)
        if chrom in NAMES:
            tri.append((NAMES.index(chrom), iv[0][0], iv[0][1]))
    want, _ = engine.count(np.array(tri, dtype=np.int32), None, gtx.READS_SORTED)
    rules = gtx.TextRules.make(NAMES, sorted_rules=True)
    text = ("\n".join(body) + "\n").encode()
    hits, info, verdicts = engine.count_text([text[: len(text) // 2 + text[len(text) // 2:].index(b"\n") + 1],
                                              text[len(text) // 2 + text[len(text) // 2:].index(b"\n") + 1:]],
                                             rules, gtx.READS_SORTED, sam=True)
    assert verdicts == [0, 0]
    assert np.array_equal(hits, want)
    # the same block with one spliced alignment in it comes back, uncounted
    odd = body[:100] + ["\t".join(body[100].split("\t")[:5] + ["5M5N5M"] + body[100].split("\t")[6:9] + ["*", "*"])] + body[101:]
    hits2, _, verdicts2 = engine.count_text([("\n".join(odd) + "\n").encode()], rules, gtx.READS_SORTED, sam=True)
    assert verdicts2 == [1] and int(hits2.sum()) == 0
