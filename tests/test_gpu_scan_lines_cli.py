"""`genomic_scans counts` with its output lines rendered on the device (GTX_SCAN_LINES_ON_DEVICE=2: an error where the host loop would
run, so that no run here can pass on the fallback), with the host loop (=0) and through the oracle CLI: stdout, stderr and exit code
must be equal.  The genome and the reads have the shape of tests/test_gpu_scans_filter_cli.py: three chromosomes, 30 000 reads, and
reads on a chromosome the genome file does not name."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from test_gpu_scans_filter_cli import LENGTHS, NAMES, RUNS as FILTER_RUNS, bed_lines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCANS = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc", "genomic_scans")


def product(args, cwd, lines, extra=None):
    env = dict(os.environ, **(extra or {}))
    for k in ("GTX_SCAN_LINES_ON_DEVICE", "GTX_SCAN_FILTER_ON_DEVICE", "GTX_NGPU"):
        env.pop(k, None)
    if lines is not None:
        env["GTX_SCAN_LINES_ON_DEVICE"] = lines
    r = subprocess.run([SCANS] + list(args), capture_output=True, cwd=cwd, env=env)
    return r.returncode, r.stdout.decode(), r.stderr.decode().strip()


def oracle(args, cwd):
    r = subprocess.run([orc.CLI] + list(args), capture_output=True, cwd=cwd)
    return r.returncode, r.stdout.decode(), r.stderr.decode().strip()


@pytest.fixture(scope="module")
def beds(tmp_path_factory):
    d = tmp_path_factory.mktemp("scanlines")
    rng = np.random.default_rng(53)
    with open(d / "genome.bed", "w") as f:
        for n, ln in zip(NAMES, LENGTHS):
            f.write("%s\t0\t%d\n" % (n, ln))
    n = 30000
    c = rng.choice(4, size=n, p=[0.58, 0.3, 0.1, 0.02])                          # class 3: a chromosome the genome file does not name
    s = (rng.random(n) ** 2 * (np.asarray(LENGTHS + [50000])[c] - 40)).astype(np.int64) + 1
    m = rng.integers(0, 2, size=n)
    rows = np.stack([c, m, s, s + 35], axis=1)
    names = np.asarray(NAMES + ["chrU"])
    by_pos = rows[np.lexsort((rows[:, 2], names[rows[:, 0]]))]
    by_strand = rows[np.lexsort((rows[:, 2], rows[:, 1], names[rows[:, 0]]))]
    (d / "reads_shuffled.bed").write_text("\n".join(bed_lines(rows.tolist())) + "\n")
    (d / "reads_pos.bed").write_text("\n".join(bed_lines(by_pos.tolist())) + "\n")
    (d / "reads_strand.bed").write_text("\n".join(bed_lines(by_strand.tolist())) + "\n")
    lines = bed_lines(by_pos.tolist())
    k = int(np.flatnonzero((by_pos[1:, 0] == 0) & (by_pos[:-1, 0] == 0) & (by_pos[1:, 2] > by_pos[:-1, 2] + 5))[6000])
    lines[k], lines[k + 1] = lines[k + 1], lines[k]
    (d / "reads_pos_broken.bed").write_text("\n".join(lines) + "\n")
    refs = []
    for _ in range(80):
        cc = int(rng.integers(0, 3))
        ss = int(rng.integers(1, LENGTHS[cc]))
        refs.append((cc, int(rng.integers(0, 2)), ss, ss + int(rng.integers(0, 3000))))
    refs += [(0, 0, 250001, 330000), (2, 1, 100, 20000), (3, 0, 5, 500), (0, 0, 1, 1)]
    (d / "refs.bed").write_text("\n".join(bed_lines(refs)) + "\n")
    return d


G = ["-g", "genome.bed"]
RUNS = [
    ["counts"] + G + ["-w", "500", "-d", "25", "-min", "0", "reads_shuffled.bed"],
    ["counts"] + G + ["-w", "500", "-d", "25", "reads_shuffled.bed"],                                    # the default -min
    ["counts"] + G + ["-w", "500", "-d", "25", "-min", "100000", "reads_shuffled.bed"],                   # above every value
    ["counts", "-i"] + G + ["-w", "500", "-d", "25", "-min", "0", "reads_shuffled.bed"],
    ["counts", "-i"] + G + ["-w", "1000", "-d", "1000", "-min", "0", "reads_pos.bed"],
    ["counts"] + G + ["-w", "1000", "-d", "1000", "-min", "5", "reads_shuffled.bed"],
    ["counts", "-S"] + G + ["-w", "500", "-d", "25", "-min", "1", "reads_strand.bed"],
    ["counts", "-S", "-i"] + G + ["-w", "500", "-d", "25", "-min", "12", "reads_pos.bed"],
    ["counts", "-S", "-i"] + G + ["-w", "1000", "-d", "1000", "-min", "0", "reads_pos.bed"],
    ["counts", "-op", "c"] + G + ["-w", "500", "-d", "25", "-min", "3", "reads_shuffled.bed"],
    ["counts", "-i", "-op", "c"] + G + ["-w", "1000", "-d", "1000", "-min", "0", "reads_shuffled.bed"],
]
BROKEN = [["counts", "-S", "-i"] + G + ["-w", "500", "-d", "25", "-min", "1", "reads_pos_broken.bed"],
          ["counts", "-S", "-i"] + G + ["-w", "1000", "-d", "1000", "-min", "0", "reads_pos_broken.bed"]]


def ident(a):
    return " ".join(a[1:])


def three_ways(args, beds):
    want = oracle(args, beds)
    got = product(args, beds, "2")
    host = product(args, beds, "0")
    assert got == want
    assert host == want
    return want


@pytest.mark.parametrize("args", RUNS, ids=[ident(a) for a in RUNS])
def test_lines_on_the_device_equal_the_host_loop_and_the_oracle_cli(beds, args):
    want = three_ways(args, beds)
    assert want[0] == 0 and want[2] == ""
    if "100000" in args:
        assert want[1] == ""
    else:
        assert len(want[1].splitlines()) > 100
    assert "chrU" not in want[1]


@pytest.mark.parametrize("args", BROKEN, ids=[ident(a) for a in BROKEN])
def test_a_broken_sorted_input_prints_a_prefix_of_the_lines_then_the_error(beds, args):
    want = three_ways(args, beds)
    assert want[0] != 0 and want[2] != "" and len(want[1].splitlines()) > 10
    whole = oracle(args[:-1] + ["reads_pos.bed"], beds)
    assert whole[0] == 0 and whole[1].startswith(want[1]) and len(whole[1]) > len(want[1])


@pytest.mark.parametrize("args", FILTER_RUNS, ids=[ident(a) for a in FILTER_RUNS])
def test_filtered_lines_on_the_device(beds, args):
    want = three_ways(args, beds)
    assert want[0] == 0


def test_filtered_broken_input(beds):
    want = three_ways(["counts", "-S", "-i"] + G + ["-r", "refs.bed", "-w", "500", "-d", "25", "-min", "1", "reads_pos_broken.bed"], beds)
    assert want[0] != 0 and len(want[1].splitlines()) > 3


FALLBACKS = [["counts", "-Sref", "-i"] + G + ["-r", "refs_sorted.bed", "-w", "500", "-d", "25", "-min", "8", "reads_shuffled.bed"],
             ["counts", "--ngpu", "2"] + G + ["-w", "500", "-d", "25", "-min", "8", "reads_shuffled.bed"]]


@pytest.mark.parametrize("args", FALLBACKS, ids=[ident(a) for a in FALLBACKS])
def test_what_falls_back_says_so_under_2_and_prints_the_host_bytes_otherwise(beds, args):
    if "-Sref" in args and not os.path.exists(beds / "refs_sorted.bed"):
        rows = sorted(line.split("\t") for line in (beds / "refs.bed").read_text().splitlines())
        rows.sort(key=lambda r: (r[0], int(r[1])))
        (beds / "refs_sorted.bed").write_text("\n".join("\t".join(r) for r in rows) + "\n")
    rehearse = {"GTX_GROUP_REHEARSE": "1"}                                        # (the library's test mode: both members on one device)
    strict = product(args, beds, "2", rehearse)
    assert strict[0] != 0 and strict[1] == "" and "would fall back to the host loop" in strict[2]
    unset, off = product(args, beds, None, rehearse), product(args, beds, "0", rehearse)
    assert unset[0] == 0 and unset == off and len(unset[1].splitlines()) > 50
    want = oracle([a for a in args if a not in ("--ngpu", "2")], beds)
    assert unset[1] == want[1]


def test_a_chromosome_name_beyond_the_limit_keeps_the_host_loop(tmp_path):
    long_name = "scaffold_" + "x" * 48                                           # longer than GTX_LINES_MAX_NAME
    (tmp_path / "genome.bed").write_text("chr1\t0\t20000\n%s\t0\t9000\n" % long_name)
    rng = np.random.default_rng(59)
    s = rng.integers(0, 8000, size=3000)
    (tmp_path / "reads.bed").write_text("".join("%s\t%d\t%d\tr\t0\t%s\n" % (("chr1", long_name)[k % 2], a, a + 36, "+-"[k % 3 == 0]) for k, a in enumerate(s.tolist())))
    args = ["counts", "-g", "genome.bed", "-w", "500", "-d", "25", "-min", "3", "reads.bed"]
    want = oracle(args, tmp_path)
    assert want[0] == 0 and long_name in want[1]
    assert product(args, tmp_path, None) == want and product(args, tmp_path, "0") == want
    strict = product(args, tmp_path, "2")
    assert strict[0] != 0 and strict[1] == "" and "would fall back to the host loop" in strict[2]
    for extra in (["-i"], ["-r", "refs.bed"]):                                   # ... and so does the filter's output
        (tmp_path / "refs.bed").write_text("chr1\t100\t5000\tr\t0\t+\n%s\t10\t3000\tr\t0\t-\n" % long_name)
        run = args[:1] + extra + args[1:]
        want = oracle(run, tmp_path)
        assert want[0] == 0 and product(run, tmp_path, None) == want
        assert "would fall back to the host loop" in product(run, tmp_path, "2")[2]
