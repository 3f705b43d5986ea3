"""The restatement of the line renderer (tests/window_lines_cases.py) pinned without a GPU: its constants against the sources, render
against lines written out by hand, and against the oracle CLI's `counts` output for window values from the oracle's scanner."""
import os
import re
import subprocess

import numpy as np

from oracle import orc

import window_lines_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ibm-cbc-genomic-tools_amd", "csrc")


def constant(text, name):
    m = re.search(r"\b%s\s*=\s*([0-9a-zA-Z_ *+]+?)\s*[,;]" % name, text)
    assert m, name
    return m.group(1)


def test_constants_are_the_sources():
    import gtx
    h = open(os.path.join(CSRC, "gtx_lines.h")).read()
    assert int(constant(h, "kLinesRow")) == W.ROW
    assert int(constant(h, "kLinesRows")) * W.ROW == W.TILE
    assert int(constant(h, "kLinesThreads")) // 64 == W.BLOCK_TILES
    assert int(constant(h, "kLinesMaxName")) == W.MAX_NAME
    api = open(os.path.join(ROOT, "include", "gtx.h")).read()
    assert int(re.search(r"#define GTX_LINES_TILE (\d+)", api).group(1)) == W.TILE == gtx.LINES_TILE
    assert int(re.search(r"#define GTX_LINES_MAX_NAME (\d+)", api).group(1)) == W.MAX_NAME == gtx.LINES_MAX_NAME
    assert int(re.search(r"#define GTX_E_SINK\s+(-\d+)", api).group(1)) == gtx.E_SINK
    k = open(os.path.join(CSRC, "gtx_lines.hip")).read()
    assert "16 * 64" in k and "uint32x4" in k and W.UNIT == 16              # the emit pass stores units of 16 bytes, one per lane


def test_render_by_hand():
    lay = W.Layout([0, 3, 3, 5], ["chr1", "chr1", "chrX"], "+-+", 25, 500)
    v = np.array([12, 3, 0, (1 << 64) - 2, 7], dtype=np.uint64)
    assert W.render(v, lay, 0, 5) == (b"12\tchr1 + 1 500\n3\tchr1 + 26 525\n0\tchr1 + 51 550\n7\tchrX + 26 525\n", 4, -1)
    assert W.render(v, lay, -5, 5) == (b"12\tchr1 + 1 500\n3\tchr1 + 26 525\n0\tchr1 + 51 550\n-2\tchrX + 1 500\n7\tchrX + 26 525\n", 5, -1)
    assert W.render(v, lay, 4, 5) == (b"12\tchr1 + 1 500\n7\tchrX + 26 525\n", 2, -1)
    assert W.render(v, lay, 0, 2) == (b"12\tchr1 + 1 500\n3\tchr1 + 26 525\n", 2, -1)
    assert W.render(v, lay, 0, 5, first=1, count=2) == (b"3\tchr1 + 26 525\n0\tchr1 + 51 550\n", 2, -1)
    v[2] = W.ONES
    assert W.render(v, lay, -5, 5) == (b"12\tchr1 + 1 500\n3\tchr1 + 26 525\n", 2, 2)
    assert W.render(v, lay, 100, 5) == (b"", 0, 2)                            # whatever min_value is
    o = np.array([0, 3, 4], dtype=np.int64)
    pv = np.array([5, 1 << 63, 9], dtype=np.uint64)
    assert W.render_pairs(o, pv, lay, 5) == (b"5\tchr1 + 1 500\n9\tchrX + 26 525\n", 2, -1)
    assert W.render_pairs(o, pv, lay, 4) == (b"5\tchr1 + 1 500\n", 1, -1)
    pv[1] = W.ONES
    assert W.render_pairs(o, pv, lay, 5) == (b"5\tchr1 + 1 500\n", 1, 3)
    assert lay.max_bytes() == 20 + 1 + 4 + 3 + 2 + 1 + 3 + 1


def test_the_case_families_hold_what_they_aim_at():
    assert len(W.all_cases()) > 40 and len(W.pair_cases()) > 30


NAMES = ["chr1", "chr2", "chrX"]
LENGTHS = [9000, 3100, 700]


def oracle_counts(tmp_path, ignore_strand, step, size, min_value):
    rng = np.random.default_rng(23)
    n = 4000
    c = rng.choice(3, size=n, p=[0.6, 0.3, 0.1])
    s = (rng.random(n) ** 2 * (np.asarray(LENGTHS)[c] - 40)).astype(np.int64) + 1
    m = rng.integers(0, 2, size=n)
    with open(tmp_path / "genome.bed", "w") as f:
        for name, ln in zip(NAMES, LENGTHS):
            f.write("%s\t0\t%d\n" % (name, ln))
    with open(tmp_path / "reads.bed", "w") as f:
        for k in range(n):
            f.write("%s\t%d\t%d\tr%d\t0\t%s\n" % (NAMES[c[k]], s[k] - 1, s[k] + 35, k, "+-"[m[k]]))
    args = ["counts"] + (["-i"] if ignore_strand else []) + ["-g", "genome.bed", "-w", str(size), "-d", str(step), "-min", str(min_value), "reads.bed"]
    r = subprocess.run([orc.CLI] + args, capture_output=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    # the same windows from the oracle's scanner, its classes in the blocks' order: chromosome-major, the strand inner
    ns = 1 if ignore_strand else 2
    cls = c * ns + (0 if ignore_strand else m)
    reads = np.stack([cls, s, s + 35], axis=1).astype(np.int32)
    win, off = orc.scan(reads, np.repeat(LENGTHS, ns), step, size)
    lay = W.Layout(list(off) + [len(win)], [NAMES[b // ns] for b in range(3 * ns)], "".join("+-"[b % ns] for b in range(3 * ns)), step, size)
    return r.stdout, win, lay


def test_render_is_the_oracle_cli_stranded(tmp_path):
    want, win, lay = oracle_counts(tmp_path, False, 25, 500, 100)
    text, lines, end = W.render(win, lay, 100, lay.total)
    assert text == want and end == -1 and 0 < lines < lay.total and b" - " in text and b"chrX" in text


def test_render_is_the_oracle_cli_ignoring_strand(tmp_path):
    want, win, lay = oracle_counts(tmp_path, True, 1000, 1000, 0)
    text, lines, end = W.render(win, lay, 0, lay.total)
    assert text == want and lines == lay.total == 9 + 3 + 0 and b" - " not in text
