"""The line renderer (csrc/gtx_lines.hip) restated in plain Python integers, and the case families its tests run: what
`genomic_scans counts` prints for a window vector (render: GenomicRegionSetScanner::PrintRemaining) and for the (ordinal, value) pairs
the window filter keeps (render_pairs: PrintFiltered).  Every family ends in an assertion of what it aims at, so that a change of a
constant that moves a seam away from under a case is noticed here and not by a test that has quietly stopped testing it."""
import bisect

import numpy as np

# the kernel's constants (tests/test_window_lines_cases_cpu.py compares them with the sources)
ROW = 128                  # entries of a row: two per lane
TILE = 1024                # entries of a wave's tile: eight rows; ranges of the host entry are cut at multiples of it
BLOCK_TILES = 4            # waves of a block
MAX_NAME = 48              # the longest name a layout may hold
UNIT = 16                  # bytes of an aligned store of the emit pass
ONES = (1 << 64) - 1


class Layout:
    def __init__(self, block_offset, names, strands, step, size):
        self.block_offset = [int(x) for x in block_offset]          # n_blocks + 1
        self.names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        self.strands = strands
        self.step, self.size = int(step), int(size)
        assert len(self.names) == len(self.block_offset) - 1 == len(strands) and self.block_offset[0] == 0

    @property
    def total(self):
        return self.block_offset[-1]

    def block_of(self, at):
        """empty blocks share an offset: the last block at or below the ordinal holds it"""
        return bisect.bisect_right(self.block_offset, at, 0, len(self.names)) - 1

    def max_bytes(self):
        m = 0
        for b, name in enumerate(self.names):
            k = max(self.block_offset[b + 1] - self.block_offset[b] - 1, 0)
            m = max(m, 20 + 1 + len(name) + 3 + len(str(self.step * k + 1)) + 1 + len(str(self.step * k + self.size)) + 1)
        return m

    def line(self, at, value):
        b = self.block_of(at)
        k = at - self.block_offset[b]
        v = int(value)
        v = v - (1 << 64) if v >= (1 << 63) else v
        return b"%d\t%s %s %d %d\n" % (v, self.names[b], self.strands[b].encode(), self.step * k + 1, self.step * k + self.size)


def _signed(v):
    v = int(v)
    return v - (1 << 64) if v >= (1 << 63) else v


def render(values, layout, min_value, limit, first=0, count=None):
    """-> (text, lines, end_at): the vector rule over windows [first, first + count)"""
    count = len(values) - first if count is None else count
    out, n = [], 0
    for i in range(first, first + count):
        if i >= limit:
            break
        if int(values[i]) == ONES:
            return b"".join(out), n, i
        if _signed(values[i]) >= min_value:
            out.append(layout.line(i, values[i])); n += 1
    return b"".join(out), n, -1


def render_pairs(ordinals, values, layout, limit, first=0, count=None):
    """-> (text, lines, end_at): the pair rule over entries [first, first + count)"""
    count = len(values) - first if count is None else count
    limit = min(limit, layout.total)
    out, n = [], 0
    for j in range(first, first + count):
        at = int(ordinals[j])
        if at < 0 or at >= limit:
            continue
        if int(values[j]) == ONES:
            return b"".join(out), n, at
        if _signed(values[j]) >= 0:
            out.append(layout.line(at, values[j])); n += 1
    return b"".join(out), n, -1


# ---- layouts ----
def one_block(n, name="chr1", strand="+", step=25, size=500):
    return Layout([0, n], [name], strand, step, size)


def stranded(lengths, names, step=25, size=500):
    """the scanner's blocks: chromosome-major, '+' then '-'"""
    off, nm, st = [0], [], ""
    for ln, name in zip(lengths, names):
        for s in "+-":
            off.append(off[-1] + ln); nm.append(name); st += s
    return Layout(off, nm, st, step, size)


def case(name, layout, values, min_value=0, limit=None, first=0, count=None):
    values = np.asarray(values, dtype=np.uint64)
    count = len(values) - first if count is None else count
    return dict(name=name, layout=layout, values=values, min_value=min_value, limit=layout.total if limit is None else limit, first=first, count=count)


def sizes_and_tiles():
    """n at the row, the wave tile and the block of four tiles; first and count that start and end inside tiles"""
    rng = np.random.default_rng(7)
    ns = [1, 2, ROW - 1, ROW, ROW + 1, TILE - 1, TILE, TILE + 1, BLOCK_TILES * TILE - 1, BLOCK_TILES * TILE, BLOCK_TILES * TILE + 1]
    out = [case("n=%d" % n, one_block(n), rng.integers(0, 40, n), min_value=10) for n in ns]
    n = BLOCK_TILES * TILE + 1
    v = rng.integers(0, 40, n)
    for first, count in ((1, n - 1), (ROW + 3, 2 * TILE), (TILE - 1, 2), (TILE, TILE), (2 * TILE + 77, TILE + 5), (n - 1, 1), (5, 0)):
        out.append(case("first=%d count=%d" % (first, count), one_block(n), v, min_value=10, first=first, count=count))
    assert ns == [1, 2, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097]
    assert any(c["first"] % TILE and (c["first"] + c["count"]) % TILE and c["first"] // TILE != (c["first"] + c["count"]) // TILE for c in out)
    assert any(c["first"] % 2 for c in out)                                       # an odd first: the pair load begins in front of the range
    return out


def value_digits():
    """every digit count of a value, 2^63 - 1, and 2^63 (negative as signed) under a negative min_value and under 0"""
    vals = [0]
    for d in range(1, 19):
        vals += [10 ** d - 1, 10 ** d]
    vals += [(1 << 63) - 1, 1 << 63, (1 << 64) - 2]
    lay = one_block(len(vals))
    out = [case("digits min=-2^63", lay, vals, min_value=-(1 << 63)), case("digits min=0", lay, vals, min_value=0), case("digits min=-1", lay, vals, min_value=-1)]
    text = render(np.asarray(vals, dtype=np.uint64), lay, -(1 << 63), lay.total)[0]
    assert b"-9223372036854775808\t" in text and b"\n9223372036854775807\t" in text and b"\n-2\t" in text
    assert b"-" not in render(np.asarray(vals, dtype=np.uint64), lay, 0, lay.total)[0].replace(b" - ", b"")
    assert sorted({len(str(v)) for v in vals if v < 1 << 63}) == list(range(1, 20))
    return out


class SparseVec:
    """a long vector that is zero outside [start, start + len(part)): the tests make it on the device without a host copy"""
    def __init__(self, n, start, part):
        self.n, self.start, self.part = int(n), int(start), np.asarray(part, dtype=np.uint64)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.part[i - self.start] if self.start <= i < self.start + len(self.part) else np.uint64(0)


def coordinate_digits():
    """start and stop cross every power of ten up to 10^9 (999 999 976 -> 1 000 000 001 at step 25) inside one row: the block begins
    37 windows into the vector, so that neither crossing falls on a row's first window"""
    out = []
    for d in range(1, 10):
        step, size = (25, 500) if d > 3 else (1, 2)
        k = (10 ** d - 1) // step + 1                                            # the first window whose start has d + 1 digits
        n = 37 + k + 40
        first = max(37 + k - 60, 0)
        part = np.full(n - first, 3, dtype=np.uint64)
        lay = Layout([0, 37, n], ["chrA", "chr1"], "++", step, size)
        c = dict(name="coordinates 10^%d" % d, layout=lay, values=SparseVec(n, first, part), min_value=1, limit=n, first=first, count=n - first)
        out.append(c)
        text = [t.split(b" ") for t in render(c["values"], lay, 1, n, first, n - first)[0].split(b"\n") if t and b"chr1" in t]
        starts, stops = [len(t[2]) for t in text], [len(t[3]) for t in text]
        assert {d, d + 1} <= set(starts) and {d, d + 1} <= set(stops)
        for col in (starts, stops):                                              # the crossing lies inside a row
            at = first + (len(render(c["values"], lay, 1, n, first, n - first)[0].split(b"\n")) - 1 - len(text)) + col.index(d + 1)
            assert at % ROW != 0
    assert b" 999999976 " in render(out[-1]["values"], out[-1]["layout"], 1, 10 ** 10, out[-1]["first"], out[-1]["count"])[0]
    assert b" 1000000001 " in render(out[-1]["values"], out[-1]["layout"], 1, 10 ** 10, out[-1]["first"], out[-1]["count"])[0]
    return out


def keep_patterns():
    n = 2 * TILE + 37
    lay = one_block(n)
    pats = {"none": np.zeros(n), "all": np.ones(n), "alternating": np.arange(n) % 2, "first of a tile": (np.arange(n) % TILE == 0),
            "last of a tile": (np.arange(n) % TILE == TILE - 1), "one in the last partial row": (np.arange(n) == n - 2)}
    out = [case("keep " + k, lay, p.astype(np.uint64) * 7, min_value=1) for k, p in pats.items()]
    assert [render(c["values"], lay, 1, n)[1] for c in out] == [0, n, n // 2, 3, 2, 1]
    assert (n - 2) // ROW == (n - 1) // ROW and n % ROW != 0
    return out


def blocks():
    rng = np.random.default_rng(11)
    out = []
    # a seam inside a row, one exactly at a tile boundary, empty blocks sharing an offset at a seam and at the very end, + and -
    lay = Layout([0, 70, 70, 70, TILE, TILE + 300, TILE + 300, TILE + 300], ["chr1", "chr1", "chr10", "chr2", "chrX", "chrY", "chrY"], "+-+-+-+", 25, 500)
    out.append(case("seams and empty blocks", lay, rng.integers(1, 99, lay.total), min_value=1))
    assert lay.block_of(69) == 0 and lay.block_of(70) == 3 and lay.block_of(TILE) == 4 and lay.block_of(lay.total - 1) == 4 and 70 % ROW
    # 300 blocks of one window each: more blocks than a row has lanes
    lay = Layout(list(range(301)), ["s%d" % b for b in range(300)], "+-" * 150, 10, 10)
    out.append(case("300 blocks of one window", lay, rng.integers(1, 99, 300), min_value=1))
    assert len(lay.names) > ROW // 2
    lay = stranded([1500, 700, 3], ["chr1", "chr2", "chrX"], 1000, 1000)
    out.append(case("stranded three chromosomes", lay, rng.integers(0, 30, lay.total), min_value=10))
    return out


def names():
    rng = np.random.default_rng(13)
    out = []
    for ln in (1, 15, 16, 17, MAX_NAME):
        lay = Layout([0, 200, 400], ["a" * ln, "b" * ln], "+-", 25, 500)
        out.append(case("name of %d" % ln, lay, rng.integers(1, 99, 400), min_value=1))
    assert out[-1]["layout"].max_bytes() == 20 + 1 + MAX_NAME + 3 + 4 + 1 + 4 + 1
    return out


def ends_and_limits():
    rng = np.random.default_rng(17)
    n = TILE + 300
    lay = one_block(n)
    out = []
    for at in (0, TILE // 2 + 3, n - 1):
        v = rng.integers(1, 99, n).astype(np.uint64)
        v[at] = ONES
        out.append(case("all-ones at %d" % at, lay, v, min_value=1))
        out.append(case("all-ones at %d, min_value above it" % at, lay, v, min_value=50))
        assert render(v, lay, 50, n)[2] == at
    v = rng.integers(1, 99, n).astype(np.uint64)
    v[700] = ONES; v[300] = ONES
    out.append(case("two all-ones: the first ends", lay, v, min_value=1))
    out.append(case("all-ones behind the limit does not end", lay, v, min_value=1, limit=300))
    out.append(case("all-ones in front of first does not end", lay, v, min_value=1, first=301, count=200))
    assert render(v, lay, 1, n)[2] == 300 and render(v, lay, 1, 300)[2] == -1 and render(v, lay, 1, n, 301, 200)[2] == -1
    v = rng.integers(1, 99, n).astype(np.uint64)
    for limit in (0, ROW + 61, n):
        out.append(case("limit %d" % limit, lay, v, min_value=1, limit=limit))
    assert (ROW + 61) % ROW and render(v, lay, 1, 0)[0] == b""
    return out


FAMILIES = [sizes_and_tiles, value_digits, coordinate_digits, keep_patterns, blocks, names, ends_and_limits]


def all_cases():
    return [c for f in FAMILIES for c in f()]


def pair_cases():
    """(name, layout, ordinals, values, limit, first, count): the same families through the pair rule -- ordinals strictly increasing,
    gaps of many tiles, all in one block, and the vector cases' kept windows as pairs"""
    rng = np.random.default_rng(19)
    out = []
    for c in all_cases():
        if c["first"] or c["count"] != len(c["values"]) or isinstance(c["values"], SparseVec):
            continue
        v, lay = c["values"], c["layout"]
        keep = np.flatnonzero((v.astype(np.int64) >= c["min_value"]) | (v == np.uint64(ONES)))
        out.append(dict(name="pairs of " + c["name"], layout=lay, ordinals=keep.astype(np.int64), values=v[keep], limit=c["limit"], first=0, count=len(keep)))
    lay = stranded([2000 * TILE, 9 * TILE, 100], ["chr1", "chr2", "chrX"])
    o = np.sort(rng.choice(lay.total, 3000, replace=False)).astype(np.int64)
    out.append(dict(name="gaps of many tiles", layout=lay, ordinals=o, values=rng.integers(0, 1 << 40, 3000).astype(np.uint64), limit=lay.total, first=0, count=3000))
    assert np.all(np.diff(o) > 0) and np.max(np.diff(o)) > 2 * TILE
    out.append(dict(name="gaps, a range inside", layout=lay, ordinals=o, values=out[-1]["values"], limit=o[2500], first=TILE + 1, count=TILE + 500))
    lay1 = one_block(50 * TILE)
    o1 = np.sort(rng.choice(lay1.total, 2 * TILE + 3, replace=False)).astype(np.int64)
    v1 = rng.integers(0, 1000, len(o1)).astype(np.uint64)
    v1[5] = 1 << 63                                                                # negative as signed: dropped
    out.append(dict(name="all in one block", layout=lay1, ordinals=o1, values=v1, limit=lay1.total, first=0, count=len(o1)))
    assert render_pairs(o1, v1, lay1, lay1.total)[1] == len(o1) - 1
    return out


def chunk_bound(layout):
    """the bytes of bound of one tile: the smallest chunk the host entry takes"""
    return TILE * layout.max_bytes()
