"""The device GFF tokenizer (text_parse_kernel<kFmtGff>, parse_gff_line of csrc/gtx_text.hip) at every block, tile and byte seam and at
every field edge, through the C ABI (gtx_count_add_text and its kin with GTX_TEXT_GFF).

The observable, the four assertions per case and the harness are those of tests/test_gpu_text_seams.py, given the GFF flag and
tests/gff_cases.py (pinned to the host packer, to tests/gff_text.py and to the oracle's CLI by tests/test_gff_cases_cpu.py):
  (a) a block whose restated result is ERROR (a '.' strand in a strand-aware run included: it is the host's to report) has a verdict != 0
  (b) whenever every verdict is 0 the hits equal the expected depth exactly
  (c) a block that comes back is counted nowhere
  (d) a clean block, or one whose probe is in the plain case documented at GTX_TEXT_GFF in include/gtx.h, has verdict 0
and on top of them (e): a block with a probe outside that plain case comes back -- needs_host exactly when the restatement says
not plain -- wherever the probe's line is one no later line can make up for.
"""
import functools

import numpy as np
import pytest

import gtx
import gff_cases as gc
import text_cases as tc
from oracle import orc
from test_gpu_text_seams import BIG_LO, Rules, Unit, _forget_refs, check, claims, oracle_agrees, set_unit_refs, strand_patterns      # noqa: F401

pytestmark = pytest.mark.gpu

N = len(tc.NAMES)


def R(mode, aware=False, by_strand=False, max_label=1, names=tc.NAMES):
    return Rules(mode, aware, by_strand, max_label, names, sam=gtx.TEXT_GFF, cases=gc)      # (the shared harness hands `sam` on as its one format argument: a format flag stands for itself)


# probes that are not plain only where the label is read (max_label > 1), or only for a mode's validity rules: what the device does
# with them depends on the rules, so (e) leaves them out
_RULE_DEPENDENT = {"label-19-digits", "label-int32-min-1", "label-control-byte", "end-0", "start-above-end", "zero-length"}


def probe_unit(p, j, n, **kw):
    """a probe in the plain case must stay (d); one outside it must come back (e)"""
    back = p is not None and not p.plain and p.group != "order" and p.name not in _RULE_DEPENDENT
    return Unit(gc.place(p, j, n, **kw), (p, j, n), stay=p is None or p.plain, back=back)


CONFIGS = [R(m, aware=a, max_label=l) for m in ("ou", "os") for a in (False, True) for l in (1, 5)]
CONFIG_IDS = ["%s%s%s" % (c.mode, "-strands" if c.aware else "", "-labels" if c.max_label > 1 else "") for c in CONFIGS]


@functools.lru_cache(maxsize=None)
def position_units(big):
    """every probe at every line position of a 300-line block (the same text for the eight configurations)"""
    return [probe_unit(p, j, 300) for p in gc.PROBES if p.big == big for j in tc.LINE_POSITIONS]


@pytest.mark.parametrize("rules", CONFIGS, ids=CONFIG_IDS)
def test_probe_at_every_line_position(engine, rules):
    """every probe at lines 0, 1, 63, 64, 127, 128, 129, 255, 256, 257 and the last of a 300-line block: the first and last line of
    a 128-line parse block, and of each of its two waves"""
    units = position_units(False)
    verdicts, kept = check(engine, units, rules)
    assert verdicts.count(0) >= len(units) // 5 and any(verdicts)  # both outcomes are exercised
    oracle_agrees(rules, probe_unit(None, 0, 300))
    # the probes at the coordinate limit: bases 2^31 - 12 .. 2^31 - 3 of every class (END 2147483645 is kept, 2147483646 is not)
    verdicts, kept = check(engine, position_units(True), rules, lo=BIG_LO, length=10)
    if rules.mode == "ou":
        assert sum(k[2] == 2147483645 for res in kept for k in res) == 2 * len(tc.LINE_POSITIONS)
    # by strand: the '+' line behind '-' lines is late, whatever its START
    if rules.mode == "os" and rules.aware:
        by = R("os", True, True, rules.max_label)
        units = [probe_unit(gc.PROBE[p], j, 300) for p in ("strand-back", "strand-forward", "strand-minus", "strand-plus", "equal-start") for j in tc.LINE_POSITIONS]
        verdicts, _ = check(engine, units, by)
        assert 0 in verdicts and any(verdicts)


def test_the_dot_strand_is_the_hosts_with_and_without_the_strand(engine):
    """'.' and every other third strand byte: legal when the strand is ignored, an error when it is not -- the device decides
    neither, the block comes back under both"""
    names = ("strand-dot", "strand-question", "strand-1", "strand-two-bytes", "strand-minus-1", "strand-dot-8", "empty-strand")
    for rules in (R("ou"), R("os"), R("ou", True), R("os", True, True, 5)):
        units = [probe_unit(gc.PROBE[p], j, 300) for p in names for j in (0, 127, 128, 299)]
        assert all(u.back for u in units)
        verdicts, _ = check(engine, units, rules)
        assert all(verdicts)
        errors = [rules.expected(u)[0] == tc.ERROR for u in units]
        assert any(errors) == rules.aware and (rules.aware or not any(errors))


LATE_MAKER = tc.Probe("late-maker", gc.gff(c=b"{c}_x"), "an unknown chromosome that sorts behind {c}")
BEFORE = ["clean", "unknown-chromosome", "dot-strand", "4000-bytes", "4096-bytes", "4097-bytes", "5000-bytes"]


@pytest.mark.parametrize("before", BEFORE)
def test_order_check_reads_the_line_before_wherever_it_lies(engine, before):
    """the offending line at j in 1, 127, 128, 129, 256: the first line of a parse block (128, 256) has the line before it in global
    memory, every other one in LDS.  There parse_gff_line reads it again, attribute column and all; a line before of more than 4096
    bytes is too long to look at: that block comes back, or is right.  A '.' line before voids the block whatever follows."""
    fields = tc.filler_fields(300)
    for rules in (R("os"), R("os", True, True, 5)):
        units = []
        for j in (1, 127, 128, 129, 256):
            for p in gc.ORDER_PROBES + [None]:
                kw = {}
                if before == "unknown-chromosome":               # dropped, but its key alone makes line j late ({c}_x sorts behind {c})
                    kw["extra"] = {j - 1: LATE_MAKER}
                elif before == "dot-strand":
                    kw["extra"] = {j - 1: gc.PROBE["strand-dot"]}
                elif before != "clean":
                    kw["extra"] = {j - 1: gc.long_line(fields[j - 1], int(before.split("-")[0]))}
                stay = before in ("clean", "4000-bytes", "4096-bytes") and (p is None or p.plain)
                units.append(Unit(gc.place(p, j, 300, **kw), (p, j, before), stay=stay, back=before == "dot-strand"))
        verdicts, _ = check(engine, units, rules)
        errors = [rules.expected(u)[0] == tc.ERROR for u in units]
        assert sum(errors) >= 10 and all(errors) == (before == "unknown-chromosome" or (before == "dot-strand" and rules.aware))
    oracle_agrees(R("os", True, True, 5), probe_unit(None, 0, 300))


def stream_blocks(sizes):
    """consecutive blocks of one ascending stream"""
    total, out, first = sum(sizes), [], 0
    for n in sizes:
        out.append(gc.place(None, 0, n, first=first, total=total))
        first += n
    return out


def test_order_check_across_the_seam(engine):
    """prev_* filled from the last line of the block before, as the CLIs do; the first line of the next block against it (the
    have_prev seam)"""
    for rules in (R("os"), R("os", True, True, 5), R("os", True, False, 1)):
        units = []
        for sizes in ((130, 1, 128, 90), (128, 129), (1, 1, 298)):
            blocks = stream_blocks(sizes)
            for k, b in enumerate(blocks):                       # the clean stream: every block stays
                units.append(Unit(b, ("stream", sizes, k), prev=gc.seam_key(blocks[k - 1]) if k else None, stay=True))
        a, b = stream_blocks((130, 140))
        f = tc.filler_fields(140, 130, 270)[0]                   # the first line of block 2
        key = gc.seam_key(a)
        first_lines = {
            "equal key": (gc.gff(c=key[0], s=b"%d" % key[2], e=b"%d" % (key[2] + 5), st=key[1].encode()), True),
            "late by START": (gc.gff(c=key[0], s=b"%d" % (key[2] - 1), e=b"%d" % (key[2] + 5), st=key[1].encode()), False),
        }
        for name, (line, fine) in first_lines.items():
            u = Unit(gc.place(line, 0, 140, first=130, total=270), name, prev=key, stay=fine)
            assert (rules.expected(u)[0] != tc.ERROR) == fine, name
            units.append(u)
        # late by chromosome: the line before was chr2's; late by strand: a '-' line before, the same chromosome and a higher START
        units.append(Unit(b, "late by chromosome", prev=(b"chr2", "+", 1)))
        units.append(Unit(b, "not late: an earlier chromosome before", prev=(b"chr0", "-", 10 ** 6), stay=True))
        late_by_strand = Unit(b, "late by strand", prev=(f[0].encode(), "-", 1))
        assert f[4] == "+" and (rules.expected(late_by_strand)[0] == tc.ERROR) == rules.by_strand
        late_by_strand.stay = not rules.by_strand
        units.append(late_by_strand)
        # a '.' line before (the host read it, with the strand ignored or as the last line of a block it reported): '.' sorts behind '+' and '-'
        dot_before = Unit(b, "late by strand: a '.' line before", prev=(f[0].encode(), ".", 1))
        assert (rules.expected(dot_before)[0] == tc.ERROR) == rules.by_strand
        dot_before.stay = not rules.by_strand
        units.append(dot_before)
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
    oracle_agrees(R("os", True, True, 5), Unit(stream_blocks((130, 140))[1], "b"))


def short_line(size):
    """a plain feature in `size` bytes: from 18 on one of chr1 whose frame takes the rest; below that (15 is the shortest GFF line:
    eight columns of one byte) one of a chromosome "c..." no reference region has, which sorts in front of chr1"""
    name = b"chr1" if size >= 18 else b"c" * (size - 14)
    line = name + b"\ts\tf\t2\t2\t.\t+\t" + b"." * (size - 13 - len(name))
    assert len(line) == size and gc.read_feature(line) == (name, 2, 2, "+", 0)
    return line


def test_newlines_at_lane_and_segment_edges(engine):
    """the newline passes: 1 KB segments of 64 lanes x 16 bytes, a scalar tail where the block's end is no multiple of 16; probes
    straddling a 1 KiB newline segment and the 16-byte staging alignment.  The last column is padded to steer the offsets.  The
    shortest GFF line there is has 15 bytes: the first line's newline at offsets 15 and 16 is a whole feature in the first lane."""
    for rules in (R("ou", True, False, 5), R("os")):
        units = []
        probes = (None, gc.PROBE["crlf-9"], gc.PROBE["10-columns"], gc.PROBE["start-plus"], gc.PROBE["11-columns"], gc.PROBE["strand-dot"])
        for at in tc.NEWLINE_OFFSETS:
            for p in probes:
                for j in (1, 2, 9):
                    lines = tc.lines_of(gc.place(p, j, 130))
                    if at - len(lines[j]) < sum(len(l) + 1 for l in lines[:j]):
                        continue
                    for m, rs in ((16, tc.LEN_MOD_16), (1024, tc.LEN_MOD_1024)):
                        for r in rs:
                            u = probe_unit(p, j, 130, newline_at=at, total_bytes_mod=(m, r))
                            assert u.block[at:at + 1] == b"\n" and u.block[:at].count(b"\n") == j and len(u.block) % m == r
                            units.append(u)
        assert len(units) > 200
        for at in (15, 16, 31, 32, 47, 48, 63, 64):              # the first line's own newline
            for mod in ((16, 0), (16, 1), (16, 15), (1024, 0)):
                u = Unit(gc.place(short_line(at), 0, 130, total_bytes_mod=mod), ("line 0 ends at", at, mod), stay=True)
                assert u.block[at:at + 1] == b"\n" and u.block[:at].count(b"\n") == 0 and rules.expected(u)[0] != tc.ERROR
                units.append(u)
            if at <= 16:                                         # ... and a line two bytes short of its frame: 7 tokens
                cut = Unit(gc.place(short_line(at + 2)[:at], 0, 130), ("line 0 cut at", at))
                assert rules.expected(cut)[0] == tc.ERROR
                units.append(cut)
        for r in range(16):                                      # the block's own end on every remainder: the scalar tail of the last lane
            for n in (2, 128, 129):
                units.append(probe_unit(None, 0, n, total_bytes_mod=(16, r)))
            units.append(Unit(short_line(20 + r) + b"\n", ("one line", r), stay=True))
        for size in (1024, 1025):
            lines = gc.stretched([gc.filler_line(f) for f in tc.filler_fields(10)], size)
            u = Unit(b"\n".join(lines) + b"\n", ("a block of %d bytes" % size), stay=True)
            assert len(u.block) == size
            units.append(u)
        verdicts, _ = check(engine, units, rules)
        assert 0 in verdicts and any(verdicts)
    oracle_agrees(R("ou", True, False, 5), probe_unit(None, 0, 130))


def test_parse_block_at_the_staging_limit(engine):
    """128 lines of kLdsSam - 32 bytes (the staging GFF shares with SAM) stay and are right, one byte more and the block comes back;
    the same group as second parse block, its first byte at every offset modulo 16 (the staging starts at the 16-byte line below
    it); a block whose first group is over the limit and whose second is under comes back whole"""
    limit = gc.K_LDS_GFF - 32
    for rules in (R("os", True, False, 5), R("ou")):
        units = []
        for extra in (0, 1):
            lines = gc.stretched([gc.filler_line(f) for f in tc.filler_fields(128)], limit + extra)
            units.append(Unit(b"\n".join(lines) + b"\n", ("first parse block", limit + extra), stay=extra == 0, back=extra == 1))
            assert len(units[-1].block) == limit + extra
            for r in range(16):
                lines = [gc.filler_line(f) for f in tc.filler_fields(256)]
                head = sum(len(l) + 1 for l in lines[:128])
                head = gc.stretched(lines[:128], head + (r - head) % 16)
                tail = gc.stretched(lines[128:], limit + extra)
                u = Unit(b"\n".join(head + tail) + b"\n", ("second parse block", r, limit + extra), stay=extra == 0, back=extra == 1)
                assert (len(b"\n".join(head)) + 1) % 16 == r and len(u.block) == len(b"\n".join(head)) + 1 + limit + extra
                units.append(u)
        lines = [gc.filler_line(f) for f in tc.filler_fields(256)]
        units.append(Unit(b"\n".join(gc.stretched(lines[:128], limit + 1) + lines[128:]) + b"\n", "first group over, second under", back=True))
        units.append(Unit(b"\n".join(lines[:128] + gc.stretched(lines[128:], limit + 1)) + b"\n", "first group under, second over", back=True))
        # the lines themselves at their longest: one feature that fills the staging alone (an attribute column of ~70 kB), 127 short ones
        fields = tc.filler_fields(128)
        for extra in (0, 1):
            lines = [gc.filler_line(f) for f in fields]
            rest = sum(len(l) + 1 for l in lines) - len(lines[64]) - 1
            lines[64] = gc.long_line(fields[64], limit + extra - rest - 1)
            units.append(Unit(b"\n".join(lines) + b"\n", ("one long feature", limit + extra), stay=extra == 0, back=extra == 1))
            assert len(units[-1].block) == limit + extra
        verdicts, _ = check(engine, units, rules)
        assert verdicts.count(0) == 18
    oracle_agrees(R("ou"), units[0])


def test_strand_runs_group_across_waves_and_blocks(engine):
    """strand-aware, with label weights: the '-' lines are counted per wave and per parse block and grouped behind the others"""
    for rules in (R("os", True, False, 5), R("ou", True, False, 5)):
        units = []
        for n in (1, 128, 129, 300):
            for name, f in strand_patterns(n).items():
                units.append(Unit(gc.place(None, 0, n, strands=f), (name, n), stay=True))
        verdicts, kept = check(engine, units, rules)
        assert verdicts == [0] * len(units)
        assert sum(k[0] >= N for res in kept for k in res) > 1000 and sum(k[0] < N for res in kept for k in res) > 1000
        for u in units[-3:]:                                     # ... and each on its own, so that no second block can make up for the first
            check(engine, [u], rules)
        oracle_agrees(rules, units[-1])


def test_blocks_in_flight_leave_nothing_behind(engine):
    """six blocks, clean and odd in turn, through the two slots: the odd ones ('.', CRLF, 11 columns) come back and leave nothing in
    the hits, and each slot's verdict is clean again for the block after next.  Then the same with another list of names."""
    odd = [gc.PROBE["strand-dot"], gc.PROBE["crlf-9"], gc.PROBE["11-columns"]]
    for names in (tc.NAMES, tc.NAMES + ["chr3"], tc.NAMES):
        for rules in (R("os", True, False, 5, names=names), R("ou", names=names)):
            units = []
            for k in range(3):
                units.append(probe_unit(None, 0, (300, 129, 1)[k]))
                units.append(Unit(gc.place(odd[k], (1, 128, 299)[k], 300), odd[k], back=True))
            verdicts, kept = check(engine, units, rules)
            assert [v != 0 for v in verdicts] == [False, True, False, True, False, True]
            verdicts, _ = check(engine, units[::-1], rules)
            assert [v != 0 for v in verdicts] == [True, False, True, False, True, False]
    # the lines of the fourth name are dropped by the short list and counted by the long one
    line = gc.gff(c=b"chr3", s=b"5", e=b"9") + b"\n"
    for names, n in ((tc.NAMES, 0), (tc.NAMES + ["chr3"], 4)):
        rules = R("ou", names=names)
        _, kept = check(engine, [Unit(gc.place(None, 0, 50) + line, "chr3", stay=True)], rules)
        assert len(kept[0]) == 50 + (1 if n else 0)
    oracle_agrees(R("ou"), units[0])


def test_the_two_format_flags_exclude_each_other(engine):
    set_unit_refs(engine, R("ou"))
    with pytest.raises(gtx.GtxError):
        engine.count_text([gc.place(None, 0, 10)], R("ou").text_rules(), 0, fmt=gtx.TEXT_GFF | gtx.TEXT_SAM)
    hits, _, verdicts = engine.count_text([gc.place(None, 0, 10)], R("ou").text_rules(), 0, fmt=gtx.TEXT_GFF)     # (the context goes on)
    assert verdicts == [0] and int(hits.sum()) > 0


# ---- the other consumers of the tokenizer ----------------------------------------------------------------------------------
CONSUMER_PROBES = [p for p in gc.PROBES if p.group == "label" or p.name in ("8-columns", "10-columns", "unknown-chrom", "end-0-unknown", "strand-minus",
                                                                             "strand-dot", "11-columns", "nul-label-first", "start-plus")]


def test_coverage_applies_the_overlap_rules(engine):
    """coverage over unit-width regions is the depth"""
    for rules in (R("ou", False, False, 5), R("os", True, False, 5), R("ou")):
        units = [probe_unit(p, j, 200) for p in CONSUMER_PROBES + [gc.PROBE["end-0"], None] for j in (0, 128, 199)]
        verdicts, _ = check(engine, units, rules, call="coverage_text")
        assert 0 in verdicts and any(verdicts)


@pytest.mark.parametrize("max_label", (1, 5), ids=("unweighted", "weighted"))
@pytest.mark.parametrize("mode", ("su", "ss"))
def test_scans_apply_their_rules_and_sum_the_labels(engine, mode, max_label):
    """1-bp windows: the weight of every kept feature at its START.  The label sum takes every line of a block the device kept, those
    of an unknown chromosome included -- also where the last 128-line group ends inside its second wave."""
    scan_flags, algo = {"su": (0, 0), "ss": (gtx.ZERO_LENGTH_OK, 1)}[mode]
    class_len = [tc.L] * N
    rules = R(mode, False, False, max_label)
    units = [probe_unit(p, j, 200) for p in CONSUMER_PROBES + [None] for j in (0, 128, 199)]
    units += [probe_unit(None, 0, n) for n in (65, 193, 219, 127, 128, 1)]
    pieces = [(u.block, rules.text_rules(), 0) for u in units]
    win, off, labels, verdicts = engine.scan_stream(pieces, class_len, 1, 1, weighted=max_label > 1, flags=scan_flags, fmt=gtx.TEXT_GFF)
    kept, label_sum = [], 0
    for u, v in zip(units, verdicts):
        res, s = rules.expected(u)
        if res == tc.ERROR:
            assert v != 0, ("(a)", mode, u.what)
            continue
        if u.stay:
            assert v == 0, ("(d)", mode, max_label, u.what)
        if u.back:
            assert v != 0, ("(e)", mode, max_label, u.what)
        if v == 0:
            kept.append(res)
            label_sum += s
    assert verdicts.count(0) >= len(units) // 3 and any(verdicts)
    assert labels == label_sum, (mode, max_label)
    want = np.zeros(N * tc.L, dtype=np.uint64)               # (the sorted scanner takes one ordered stream: block by block)
    for res in kept:
        tri = np.array([k[:3] for k in res], dtype=np.int32).reshape(-1, 3)
        w = np.array([k[3] for k in res], dtype=np.int32) if max_label > 1 else None
        want += orc.scan(tri, class_len, 1, 1, weights=w, algo=algo)[0]
    np.testing.assert_array_equal(win, want)
    plain = [0] * (N * tc.L)                                  # ... which is, by plain accumulation, the weight of every kept line at its start
    for c, s, e, wt in (k for res in kept for k in res):
        plain[c * tc.L + s - 1] = (plain[c * tc.L + s - 1] + wt) % (1 << 64)
    assert list(win) == plain
    # each short block once more on its own, so that no other block's lines can make up for missing ones
    for u in units[-6:]:
        _, _, labels1, v1 = engine.scan_stream([(u.block, rules.text_rules(), 0)], class_len, 1, 1, weighted=max_label > 1, flags=scan_flags, fmt=gtx.TEXT_GFF)
        assert v1 == [0] and labels1 == rules.expected(u)[1], u.what


FUZZ = {"ou": (31, 120, R("ou")), "os": (32, 120, R("os")), "os-by-strand": (33, 120, R("os", True, True, 1)), "ou-weighted": (34, 120, R("ou", False, False, 5)),
        "os-strands-weighted": (35, 120, R("os", True, False, 5))}      # (tests/test_gff_cases_cpu.py holds the same seeds, counts and rules)


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_fuzz_blocks_equal_the_restatement(engine, name):
    seed, n, rules = FUZZ[name]
    units = [Unit(b, (p, j, b.count(b"\n")), stay=p is None or p.plain) for b, p, j in gc.fuzz_blocks(seed, n)]
    verdicts, kept = check(engine, units, rules)
    assert verdicts.count(0) >= n // 2
    oracle_agrees(rules, units[0])
