"""The device BED tokenizer (csrc/gtx_text.hip) at every block, tile and byte seam, through the C ABI.

The observable: a reference set with one unit-width region [p, p] for every base p of every class, so that the count vector is the
weighted depth per base and class -- any change to one line's class, start, stop or weight changes it.  The expected depth comes
from tests/text_cases.py (pinned to the host packer and the oracle's CLI by tests/test_text_cases_cpu.py), by plain accumulation.

The same four assertions for every case (`check`):
  (a) a block whose restated result is ERROR has a verdict != 0
  (b) whenever every verdict is 0 the hits equal the expected depth exactly
  (c) when some blocks come back the hits equal the depth of the other blocks alone: a block that comes back is counted nowhere
  (d) a clean block, or one whose probe is in the documented plain case of include/gtx.h, has verdict 0 (unless it is an ERROR)
The device may be more cautious than the host elsewhere; nothing more is demanded.

Many independent blocks share one count call (every block with its own rules: no line before it, or the seam key the case
states), so the hits are compared once per call; on a mismatch the blocks are counted again one by one to name the first culprit.
"""
import numpy as np
import pytest

import gtx
import text_cases as tc
from oracle import orc

pytestmark = pytest.mark.gpu

N = len(tc.NAMES)
BIG_LO = 2 ** 31 - 12                       # the large-coordinate probes' own reference set: bases BIG_LO .. 2^31 - 3


class Unit:
    """one block of a count call: its text, the seam key in front of it (None: no line before), what the case claims"""
    def __init__(self, block, what, prev=None, stay=False, back=False, garbage_prev=False):
        self.block, self.what, self.prev, self.stay, self.back, self.garbage_prev = block, what, prev, stay, back, garbage_prev


class Rules:
    """the rules of one count call; sam: the blocks are SAM alignments (GTX_TEXT_SAM); cases: the module that restates what a block
    becomes (tests/text_cases.py for BED, tests/sam_cases.py for SAM)"""
    def __init__(self, mode, aware=False, by_strand=False, max_label=1, names=tc.NAMES, sam=False, cases=tc):
        self.mode, self.aware, self.by_strand, self.max_label, self.names = mode, aware, by_strand, max_label, list(names)
        self.sam, self.cases = sam, cases
        self.sorted = mode in ("os", "ss")
        self.n_classes = len(self.names) * (2 if aware else 1)

    def text_rules(self, prev=None, garbage_prev=False):
        r = gtx.TextRules.make(self.names, strand_aware=self.aware, sorted_rules=self.sorted, sorted_by_strand=self.by_strand, max_label_value=self.max_label)
        if prev is not None:
            r.have_prev, r.prev_chrom, r.prev_strand, r.prev_start = 1, prev[0], ord(prev[1]), prev[2]
        elif garbage_prev:                                        # have_prev = 0: whatever prev_* hold must not be looked at
            r.have_prev, r.prev_chrom, r.prev_strand, r.prev_start = 0, b"zzzz", ord("-"), 2 ** 40
        return r

    def expected(self, unit):
        (res,), (s,) = self.cases.expected_blocks([unit.block], self.mode, self.names, self.aware, self.by_strand, self.max_label, prev=unit.prev)
        return res, s

    def flags(self):
        return gtx.READS_SORTED | gtx.ZERO_LENGTH_OK if self.sorted else 0


_refs_now = [None]


def set_unit_refs(engine, rules, lo=1, length=tc.L):
    key = (rules.n_classes, rules.sorted, lo, length)
    if _refs_now[0] != key:
        engine.set_refs(np.array(tc.unit_refs(rules.n_classes, length, lo), dtype=np.int32), rules.n_classes, gtx.REFS_KEEP_ZERO_LENGTH if rules.sorted else 0)
        engine.set_ref_blocks(None)
        _refs_now[0] = key


@pytest.fixture(autouse=True)
def _forget_refs():
    _refs_now[0] = None                                          # (other test files set reference sets of their own on the shared engine)
    yield
    _refs_now[0] = None


def claims(units, rules, verdicts):
    """assertions (a) and (d) per block; returns the restated results of the blocks the device kept"""
    kept = []
    for u, v in zip(units, verdicts):
        res, _ = rules.expected(u)
        if res == tc.ERROR:
            assert v != 0, ("(a) an ERROR block was taken", u.what)
        else:
            if u.stay:
                assert v == 0, ("(d) a plain block came back", u.what, v)
            if u.back:
                assert v != 0, ("this block must come back", u.what)
            if v == 0:
                kept.append(res)
    return kept


def check(engine, units, rules, lo=1, length=tc.L, call="count_text"):
    set_unit_refs(engine, rules, lo, length)
    def run(*a):
        try:
            return getattr(engine, call)(*a)
        except gtx.GtxError as e:                                # a device error: nothing more is started on that GPU in this session
            pytest.exit("%s failed: %s" % (call, e), returncode=3)
    hits, _, verdicts = run([u.block for u in units], [rules.text_rules(u.prev, u.garbage_prev) for u in units], rules.flags(), rules.sam)
    kept = claims(units, rules, verdicts)
    want = np.array(tc.depth(kept, rules.n_classes, length, lo), dtype=np.uint64)
    if not np.array_equal(hits, want):                           # (b), (c): name the first block that is counted wrongly
        for u in units:
            h1, _, v1 = run([u.block], [rules.text_rules(u.prev, u.garbage_prev)], rules.flags(), rules.sam)
            k1 = claims([u], rules, v1)
            assert np.array_equal(h1, np.array(tc.depth(k1, rules.n_classes, length, lo), dtype=np.uint64)), ("(b)/(c) wrong depth", u.what, v1)
        raise AssertionError("(b)/(c): the blocks are right one by one and wrong together")
    return verdicts, kept


def oracle_agrees(rules, unit):
    """the plain accumulation of `depth` against orc.count on the same triples, once per test"""
    res, _ = rules.expected(unit)
    assert res != tc.ERROR and len(res) > 0
    tri = np.array([k[:3] for k in res], dtype=np.int32)
    w = np.array([k[3] for k in res], dtype=np.int32) if rules.max_label > 1 else None
    if rules.sorted:                                             # (the merge takes its queries in order: class by class)
        o = np.argsort(tri[:, 0], kind="stable")
        tri, w = tri[o], None if w is None else w[o]
    got = orc.count(np.array(tc.unit_refs(rules.n_classes), dtype=np.int32), tri, w, algo=orc.SORTED_MERGE if rules.sorted else orc.BIN_INDEX)
    assert np.array_equal(got, np.array(tc.depth([res], rules.n_classes), dtype=np.uint64))


def probe_unit(p, j, n, rules, **kw):
    return Unit(tc.place(p, j, n, **kw), (p, j, n), stay=p is None or p.plain)


CONFIGS = [Rules(m, aware=a, by_strand=False, max_label=l) for m in ("ou", "os") for a in (False, True) for l in (1, 5)]
CONFIG_IDS = ["%s%s%s" % (c.mode, "-strands" if c.aware else "", "-labels" if c.max_label > 1 else "") for c in CONFIGS]


@pytest.mark.parametrize("rules", CONFIGS, ids=CONFIG_IDS)
def test_probe_at_every_line_position(engine, rules):
    """every probe at lines 0, 1, 63, 64, 127, 128, 129, 255, 256, 257 and the last of a 300-line block"""
    small = [p for p in tc.PROBES if not p.big]
    units = [probe_unit(p, j, 300, rules) for p in small for j in tc.LINE_POSITIONS]
    verdicts, kept = check(engine, units, rules)
    assert verdicts.count(0) >= len(units) // 5 and any(verdicts)  # both outcomes are exercised
    oracle_agrees(rules, probe_unit(None, 0, 300, rules))
    # the probes at the coordinate limit: bases 2^31 - 12 .. 2^31 - 3 of every class (2147483644 is kept, 2147483646 is not)
    big = [probe_unit(p, j, 300, rules) for p in tc.PROBES if p.big for j in tc.LINE_POSITIONS]
    verdicts, kept = check(engine, big, rules, lo=BIG_LO, length=10)
    if rules.mode == "ou":
        assert sum(k[1] == 2147483644 for res in kept for k in res) == len(tc.LINE_POSITIONS)
    # by strand: the '+' line behind '-' lines is late, whatever its start
    if rules.mode == "os" and rules.aware:
        by = Rules("os", True, True, rules.max_label)
        units = [probe_unit(p, j, 300, by) for p in (tc.PROBE["strand-back"], tc.PROBE["strand-minus"], tc.PROBE["equal-start"]) for j in tc.LINE_POSITIONS]
        verdicts, _ = check(engine, units, by)
        assert 0 in verdicts and any(verdicts)


@pytest.mark.parametrize("before", ["clean", "unknown-chromosome", "4000-bytes", "5000-bytes"])
def test_order_check_reads_the_line_before_wherever_it_lies(engine, before):
    """the offending line at j in 1, 127, 128, 129, 256: the first line of a parse block (128, 256) has the line before it in global
    memory, every other one in LDS.  A line before of 5000 bytes is too long to look at: that block comes back, or is right."""
    for rules in (Rules("os"), Rules("os", True, True, 5)):
        units = []
        for j in (1, 127, 128, 129, 256):
            for p in tc.ORDER_PROBES + [None]:
                kw = {}
                if before == "unknown-chromosome":               # dropped, but its key alone makes line j late ({c}_x sorts behind {c})
                    kw["extra"] = {j - 1: tc.Probe("late-maker", b"{c}_x\t{s}\t{e}", "")}
                elif before != "clean":
                    kw["stretch"] = {j - 1: int(before.split("-")[0])}
                u = Unit(tc.place(p, j, 300, **kw), (p, j, before), stay=before in ("clean", "4000-bytes") and (p is None or p.plain))
                units.append(u)
        verdicts, _ = check(engine, units, rules)
        errors = [rules.expected(u)[0] == tc.ERROR for u in units]
        assert sum(errors) >= 10 and all(errors) == (before == "unknown-chromosome")
    oracle_agrees(Rules("os", True, True, 5), probe_unit(None, 0, 300, None))


def stream_blocks(sizes, cols=7):
    """consecutive blocks of one ascending stream"""
    total, out, first = sum(sizes), [], 0
    for n in sizes:
        out.append(tc.place(None, 0, n, first=first, total=total, cols=cols))
        first += n
    return out


def test_order_check_across_the_seam(engine):
    """prev_* filled from the last line of the block before, as the CLIs do; the first line of the next block against it"""
    for rules in (Rules("os"), Rules("os", True, True, 5), Rules("os", True, False, 1)):
        units = []
        for sizes in ((130, 1, 128, 90), (128, 129), (1, 1, 300)):
            blocks = stream_blocks(sizes)
            for k, b in enumerate(blocks):                       # the clean stream: every block stays
                units.append(Unit(b, ("stream", sizes, k), prev=tc.seam_key(blocks[k - 1]) if k else None, stay=True))
        a, b = stream_blocks((130, 140))
        f = tc.filler_fields(140, 130, 270)[0]                   # the first line of block 2
        key = tc.seam_key(a)
        first_lines = {
            "equal key": (b"%s\t%d\t%d\t1\t0\t%s" % (key[0], key[2] - 1, key[2] + 5, key[1].encode()), True),
            "late by start": (b"%s\t%d\t%d\t1\t0\t%s" % (key[0], key[2] - 2, key[2] + 5, key[1].encode()), False),
        }
        for name, (line, fine) in first_lines.items():
            u = Unit(tc.place(line, 0, 140, first=130, total=270), name, prev=key, stay=fine)
            assert (rules.expected(u)[0] != tc.ERROR) == fine, name
            units.append(u)
        # late by chromosome: the line before was chr2's; late by strand: a '-' line before, the same chromosome and a higher start
        units.append(Unit(b, "late by chromosome", prev=(b"chr2", "+", 1)))
        units.append(Unit(b, "not late: an earlier chromosome before", prev=(b"chr0", "-", 10 ** 6), stay=True))
        late_by_strand = Unit(b, "late by strand", prev=(f[0].encode(), "-", 1))
        assert (rules.expected(late_by_strand)[0] == tc.ERROR) == rules.by_strand
        late_by_strand.stay = not rules.by_strand
        units.append(late_by_strand)
        # after an unknown-chromosome last line: its key counts
        units.append(Unit(b, "late after an unknown chromosome", prev=(f[0].encode() + b"_x", "+", 1)))
        units.append(Unit(b, "in order after an unknown chromosome", prev=(b"chr0_x", "+", 10 ** 6), stay=True))
        assert rules.expected(units[-2])[0] == tc.ERROR and rules.expected(units[-1])[0] != tc.ERROR
        # the name slot at its limit: 4095 bytes travel, 4096 do not
        units.append(Unit(b, "prev_chrom of 4095 bytes, in order", prev=(b"c" * 4095, "+", 10 ** 6), stay=True))
        units.append(Unit(b, "prev_chrom of 4095 bytes, late", prev=(b"d" * 4095, "+", 0)))
        units.append(Unit(b, "prev_chrom of 4096 bytes", prev=(b"c" * 4096, "+", 0), back=True))
        units.append(Unit(b, "no line before, prev_* garbage", garbage_prev=True, stay=True))
        # twice over, so that every case meets both of the two slots
        verdicts, _ = check(engine, units + units[::-1], rules)
        assert verdicts == verdicts[::-1]
    oracle_agrees(Rules("os", True, True, 5), Unit(stream_blocks((130, 140))[1], "b"))


def test_newlines_at_lane_and_segment_edges(engine):
    """the newline passes: 1 KB segments of 64 lanes x 16 bytes, a scalar tail where the block's end is no multiple of 16"""
    for rules in (Rules("ou", True, False, 5), Rules("os")):
        units = []
        probes = (None, tc.PROBE["crlf"], tc.PROBE["6-columns"], tc.PROBE["eleven-digits"])
        for at in tc.NEWLINE_OFFSETS:
            for p in probes:
                for j in (1, 2, 40):
                    line = tc.lines_of(tc.place(p, j, 130))[j]
                    if at - len(line) < 30 * j:
                        continue
                    for mod in ((16, 0), (16, 1), (16, 15), (1024, 0), (1024, 1), (1024, 1023)):
                        u = probe_unit(p, j, 130, rules, newline_at=at, total_bytes_mod=mod)
                        assert u.block[at:at + 1] == b"\n" and len(u.block) % mod[0] == mod[1]
                        units.append(u)
        for at, line in ((15, b"chr1\t2\t9\t33\t0\t+"), (16, b"chr1\t2\t9\t333\t0\t+")):      # the first line's own newline on byte 15 and 16
            for mod in ((16, 0), (16, 1), (16, 15), (1024, 0)):
                u = Unit(tc.place(line, 0, 130, total_bytes_mod=mod), ("line 0 ends at", at, mod), stay=True)
                assert u.block[at:at + 1] == b"\n" and u.block[:at].count(b"\n") == 0
                units.append(u)
        for r in range(16):                                      # the block's own end on every remainder: the scalar tail of the last lane
            for n in (2, 128, 129):
                units.append(probe_unit(None, 0, n, rules, total_bytes_mod=(16, r)))
            units.append(Unit(b"chr1\t1\t9\tx" + b"y" * r + b"\n", ("one line", r), stay=True))
        short = Unit(b"chr1\t1\t9\n", "one line shorter than 16 bytes", stay=True)
        assert len(short.block) < 16
        units.append(short)
        for size in (1024, 1025):
            lines = tc.stretched([tc.filler_line(f) for f in tc.filler_fields(30)], size)
            u = Unit(b"\n".join(lines) + b"\n", ("a block of %d bytes" % size), stay=True)
            assert len(u.block) == size
            units.append(u)
        verdicts, _ = check(engine, units, rules)
        assert 0 in verdicts and any(verdicts)
    oracle_agrees(Rules("ou", True, False, 5), probe_unit(None, 0, 130, None))


def test_parse_block_at_the_lds_limit(engine):
    """128 lines of kLdsText - 32 bytes stay and are right, one byte more and the block comes back; the same group as second parse
    block, its first byte at every offset modulo 16 (the staging starts at the 16-byte line below it)"""
    limit = tc.K_LDS_TEXT - 32
    for rules in (Rules("os", True, False, 5), Rules("ou")):
        units = []
        for extra in (0, 1):
            lines = tc.stretched([tc.filler_line(f) for f in tc.filler_fields(128)], limit + extra)
            units.append(Unit(b"\n".join(lines) + b"\n", ("first parse block", limit + extra), stay=extra == 0, back=extra == 1))
            for r in range(16):
                lines = [tc.filler_line(f) for f in tc.filler_fields(256)]
                head = sum(len(l) + 1 for l in lines[:128])
                head = tc.stretched(lines[:128], head + (r - head) % 16)
                tail = tc.stretched(lines[128:], limit + extra)
                u = Unit(b"\n".join(head + tail) + b"\n", ("second parse block", r, limit + extra), stay=extra == 0, back=extra == 1)
                assert (len(b"\n".join(head)) + 1) % 16 == r
                units.append(u)
        verdicts, _ = check(engine, units, rules)
        assert verdicts.count(0) == 17
    oracle_agrees(Rules("ou"), units[0])


def strand_patterns(n):
    one = lambda k: (lambda g: "-" if g == k else "+")
    return {"all +": lambda g: "+", "all -": lambda g: "-", "alternating": lambda g: "+-"[g % 2], "- at 63": one(63), "- at 64": one(64),
            "- at 127": one(127), "- at 128": one(128), "- on 128..255": lambda g: "-" if 128 <= g < 256 else "+",
            "+ on 128..255": lambda g: "+" if 128 <= g < 256 else "-", "- from 64": lambda g: "-" if g >= 64 else "+"}


def test_strand_runs_group_across_waves_and_blocks(engine):
    """strand-aware, with label weights: the '-' lines are counted per wave and per parse block and grouped behind the '+' lines"""
    for rules in (Rules("os", True, False, 5), Rules("ou", True, False, 5)):
        units = []
        for n in (1, 128, 129, 300):
            for name, f in strand_patterns(n).items():
                units.append(Unit(tc.place(None, 0, n, strands=f), (name, n), stay=True))
        verdicts, kept = check(engine, units, rules)
        assert verdicts == [0] * len(units)
        assert sum(k[0] >= N for res in kept for k in res) > 1000 and sum(k[0] < N for res in kept for k in res) > 1000
        for u in units[-3:]:                                     # ... and each on its own, so that no second block can make up for the first
            check(engine, [u], rules)
        oracle_agrees(rules, units[-1])


def test_blocks_in_flight_leave_nothing_behind(engine):
    """six blocks, clean and odd in turn, through the two slots: the odd ones come back and leave nothing in the hits, and each slot's
    verdict is clean again for the block after next.  Then the same with another list of names, which rebuilds the tables."""
    odd = [tc.PROBE["blanks"], tc.PROBE["crlf"], tc.PROBE["eleven-digits"]]
    for names in (tc.NAMES, tc.NAMES + ["chr3"], tc.NAMES):
        for rules in (Rules("os", True, False, 5, names=names), Rules("ou", names=names)):
            units = []
            for k in range(3):
                units.append(probe_unit(None, 0, (300, 129, 1)[k], rules))
                units.append(Unit(tc.place(odd[k], (1, 128, 299)[k], 300), odd[k], back=True))
            verdicts, kept = check(engine, units, rules)
            assert [v != 0 for v in verdicts] == [False, True, False, True, False, True] and len(kept) == 3
            verdicts, _ = check(engine, units[::-1], rules)
            assert [v != 0 for v in verdicts] == [True, False, True, False, True, False]
    # the lines of the fourth name are dropped by the short list and counted by the long one
    line = b"chr3\t5\t9\n"
    for names, n in ((tc.NAMES, 0), (tc.NAMES + ["chr3"], 4)):
        rules = Rules("ou", names=names)
        _, kept = check(engine, [Unit(tc.place(None, 0, 50) + line, "chr3", stay=True)], rules)
        assert len(kept[0]) == 50 + (1 if n else 0)
    oracle_agrees(Rules("ou"), units[0])


# ---- the other consumers of the tokenizer ----------------------------------------------------------------------------------
CONSUMER_PROBES = [p for p in tc.PROBES if p.group in ("interval", "label") or p.name in ("3-columns", "unknown-chrom")]


def test_each_consumer_applies_its_own_rules(engine):
    # coverage: over unit-width regions it is the depth, under the overlap rules
    for rules in (Rules("ou", False, False, 5), Rules("os", True, False, 5), Rules("ou")):
        units = [probe_unit(p, j, 200, rules) for p in CONSUMER_PROBES + [None] for j in (0, 128, 199)]
        verdicts, _ = check(engine, units, rules, call="coverage_text")
        assert 0 in verdicts and any(verdicts)
    # scans, 1-bp windows: the unsorted scanner drops stop <= 0 and start > stop (su), the sorted one keeps them (ss); the label sum
    # takes every line of a block the device kept, dropped ones included
    class_len = [tc.L] * N
    for mode, scan_flags, algo in (("su", 0, 0), ("ss", gtx.ZERO_LENGTH_OK, 1)):
        for max_label in (1, 5):
            rules = Rules(mode, False, False, max_label)
            units = [probe_unit(p, j, 200, rules) for p in CONSUMER_PROBES + [None] for j in (0, 128, 199)]
            pieces = [(u.block, rules.text_rules(), 0) for u in units]
            win, off, labels, verdicts = engine.scan_stream(pieces, class_len, 1, 1, weighted=max_label > 1, flags=scan_flags)
            kept, label_sum = [], 0
            for u, v in zip(units, verdicts):
                res, s = rules.expected(u)
                if res == tc.ERROR:
                    assert v != 0, ("(a)", mode, u.what)
                    continue
                if u.stay:
                    assert v == 0, ("(d)", mode, max_label, u.what)
                if v == 0:
                    kept.append(res)
                    label_sum += s
            assert verdicts.count(0) >= len(units) // 3
            assert labels == label_sum, (mode, max_label)
            want = np.zeros(N * tc.L, dtype=np.uint64)           # (the sorted scanner takes one ordered stream: block by block)
            for res in kept:
                tri = np.array([k[:3] for k in res], dtype=np.int32).reshape(-1, 3)
                w = np.array([k[3] for k in res], dtype=np.int32) if max_label > 1 else None
                want += orc.scan(tri, class_len, 1, 1, weights=w, algo=algo)[0]
            np.testing.assert_array_equal(win, want)
            plain = [0] * (N * tc.L)                            # ... which is, by plain accumulation, the weight of every kept line at its start
            for c, s, e, wt in (k for res in kept for k in res):
                plain[c * tc.L + s - 1] = (plain[c * tc.L + s - 1] + wt) % (1 << 64)
            assert list(win) == plain
    # subset: the lines with hits, byte for byte; 6-column lines, a keep pattern that changes at lines 255, 256 and 257
    rules = Rules("ou")
    n = 300
    fields = tc.filler_fields(n)
    lines = [tc.filler_line(f, cols=6) + b"\n" for f in fields]
    patterns = {"255..256": {255, 256}, "256": {256}, "0..255": set(range(256)), "257..": set(range(257, n)), "nothing": set(), "everything": set(range(n)),
                "every other": set(range(0, n, 2))}
    for name, keep in patterns.items():
        # a unit-width region at col2 + 1 of every line to keep hits that line -- and every line that reaches over that base
        refs = [(tc.NAMES.index(fields[k][0]), fields[k][1] + 1, fields[k][1] + 1) for k in sorted(keep)] or [(0, tc.L, tc.L)]
        hit = [any(c == tc.NAMES.index(f[0]) and f[1] + 1 <= p <= f[2] for c, p, _ in refs) for f in fields]
        assert name in ("nothing", "everything") or (any(hit) and not all(hit))
        engine.set_refs(np.array(refs, dtype=np.int32), N)
        engine.set_ref_blocks(None)
        for inv in (0, gtx.SUBSET_INVERT):
            want = b"".join(l for l, h in zip(lines, hit) if h != bool(inv))
            odd_block = b"".join(lines[:128]) + b"chr1 1 2\n" + b"".join(lines[128:])
            got = engine.subset_text([b"".join(lines), odd_block, b"".join(lines)], rules.text_rules(), inv)
            assert [g[0] != 0 for g in got] == [False, True, False], name
            assert got[0][1] == want and got[2][1] == want and got[1][1:] == (b"", 0), (name, inv)
            assert got[0][2] == want.count(b"\n")
    for p in CONSUMER_PROBES:                                     # the interval rules are the bin index's here: an ERROR block selects nothing
        u = probe_unit(p, 128, 300, rules, cols=6)
        (redo, out, k), = engine.subset_text([u.block], rules.text_rules(), 0)
        if rules.expected(u)[0] == tc.ERROR:
            assert redo != 0 and (out, k) == (b"", 0), p


FUZZ = {"ou": (11, 150, Rules("ou")), "os": (12, 150, Rules("os")), "os-by-strand": (13, 150, Rules("os", True, True, 1)),
        "ou-weighted": (14, 150, Rules("ou", False, False, 5))}      # (tests/test_text_cases_cpu.py holds the same seeds and counts)


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_fuzz_blocks_equal_the_restatement(engine, name):
    seed, n, rules = FUZZ[name]
    units = [Unit(b, (p, j, b.count(b"\n")), stay=p is None or p.plain) for b, p, j in tc.fuzz_blocks(seed, n)]
    verdicts, kept = check(engine, units, rules)
    assert verdicts.count(0) >= n // 2
    oracle_agrees(rules, units[0])
