"""The annotate pass (gtx_join_annotate / gtx_pair_annotate_device, include/gtx.h; kernels in csrc/gtx_annotate.hip) against the
restatement (tests/annotate_restate.py).  Genes R and their upstream regions U (the restated builder's) are one reference set of
N + M regions whose order key ranks (set, level, bin, -ordinal within the set).  Expected pairs: the oracle's `pairs` rows
(oracle/gtx_oracle.c) for R and for U written out as BED, R's first; expected values: PrintAnnotations' rule (annotate_restate.pair_value)
on each.  Offsets, ordinals and values are compared exactly.  The walk's long-segment threshold is 32 pairs (kOffSmallSeg)."""
import subprocess

import numpy as np
import pytest

import annotate_restate as ar
import gtx
from oracle import orc
from oracle.restate import NAMES, bin_keys, concat, offset_from, regions, take, triples, write_bed

pytestmark = pytest.mark.gpu

THRESHOLD = 32
COUNTS = [0, 1, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1]
SPAN = 600_000


def as_dicts(r, prefix):
    return [dict(label="%s%d" % (prefix, i), chrom=NAMES[r["chrom"][i]], strand="+-"[r["strand"][i]], s=int(r["s"][i]), e=int(r["e"][i]), line=i + 1, n_iv=1)
            for i in range(len(r["s"]))]


def as_arrays(regs):
    s = np.array([x["s"] for x in regs], dtype=np.int64); e = np.array([x["e"] for x in regs], dtype=np.int64)
    return dict(chrom=np.array([NAMES.index(x["chrom"]) for x in regs]), strand=np.array([x["strand"] == "-" for x in regs], dtype=np.int64), s=s, e=e,
                first=np.arange(len(regs) + 1, dtype=np.int64), blocks=np.stack([s, e], axis=1))


def n_overlaps(both, chrom, strand, s, e, ign):
    m = (both["chrom"] == chrom) & (both["s"] <= e) & (both["e"] >= s)
    return int((m if ign else m & (both["strand"] == strand)).sum())


def query_with(both, rng, want, ign):
    """a query that meets exactly `want` regions of the combined set: from a random start its stop grows region start by region start"""
    for _ in range(400):
        chrom, strand, s = int(rng.integers(0, 3)), int(rng.integers(0, 2)), int(rng.integers(1, SPAN // 2))
        for e in np.unique(np.concatenate(([s], both["s"][(both["chrom"] == chrom) & (both["s"] > s)]))):
            c = n_overlaps(both, chrom, strand, s, int(e), ign)
            if c == want:
                return chrom, strand, s, int(e)
            if c > want:
                break
    raise AssertionError("no query with %d pairs" % want)


class World:
    """genes, upstream regions, queries (random ones plus some with exactly COUNTS pairs and a few hundred), and per -i / strand the
    oracle's pairs in print order -- computed once per module"""

    def __init__(self, tmp):
        rng = np.random.default_rng(20261)
        self.tmp = tmp
        self.R = regions(rng, 700, SPAN, 200, 3000)
        up = ar.upstream_set(as_dicts(self.R, "r"), None, False, 1500, 1500)
        self.U = as_arrays(up)
        self.n_primary, self.both = len(self.R["s"]), concat(self.R, self.U)
        self.key = np.concatenate((bin_keys(self.R), len(self.R["s"]) + bin_keys(self.U)))
        write_bed(tmp / "R.bed", self.R, "r")
        write_bed(tmp / "U.bed", self.U, "u")
        self.cache = {}
        self.rng = rng

    def queries(self, ign):
        rng = np.random.default_rng(7 + ign)
        q = regions(rng, 3000, SPAN, 1, 6000)
        crafted = [query_with(self.both, rng, c, ign) for c in COUNTS for _ in range(8)]
        crafted += [(c, st, 1000, SPAN - 1000) for c in range(3) for st in range(2)]      # a few hundred pairs each
        extra = as_arrays([dict(chrom=NAMES[c], strand="+-"[st], s=s, e=e) for c, st, s, e in crafted])
        q = concat(q, extra)
        return take(q, np.lexsort((q["s"], q["chrom"])))

    def get(self, ign):
        if ign not in self.cache:
            q = self.queries(ign)
            write_bed(self.tmp / ("Q%d.bed" % ign), q, "q")
            rows = [[] for _ in range(len(q["s"]))]
            for n, (name, base) in enumerate((("R.bed", 0), ("U.bed", self.n_primary))):
                r = subprocess.run([orc.CLI, "pairs"] + (["-i"] if ign else []) + [name, "Q%d.bed" % ign], capture_output=True, cwd=self.tmp)
                assert r.returncode == 0, r.stderr.decode()
                for a, b in (x.split("\t") for x in r.stdout.decode().splitlines()):
                    rows[int(a) - 1].append(base + int(b[1:]))
            self.cache[ign] = (q, rows)
        return self.cache[ign]

    def expected(self, ign, mode, n_primary=None, ops=("5p", "3p")):
        """(pairs per query in print order, kept offsets, kept ordinals, kept values)"""
        q, rows = self.get(ign)
        n_primary = self.n_primary if n_primary is None else n_primary
        koff, kref, kval = [0], [], []
        for i, hits in enumerate(rows):
            for k in hits:
                so, eo = offset_from([(int(self.both["s"][k]), int(self.both["e"][k]))], self.both["strand"][k] == 1, ops[0] if k < n_primary else ops[1],
                                     int(q["s"][i]), int(q["e"][i]))
                v = so + eo if mode == gtx.ANNOTATE_CENTER else so
                if mode != gtx.ANNOTATE_CENTER or v >= 0:
                    kref.append(k); kval.append(v)
            koff.append(len(kref))
        return rows, np.array(koff, dtype=np.int64), np.array(kref, dtype=np.int32), np.array(kval, dtype=np.int64)

    def load(self, engine, ign, buffer=1 << 26):
        engine.set_refs(triples(self.both, ign), len(NAMES) * (1 if ign else 2))
        engine.set_ref_blocks(None)
        engine.set_ref_order(self.key)
        engine.set_ref_strands(self.both["strand"])
        engine.set_join_buffer(buffer)
        return triples(self.get(ign)[0], ign)


def mixed_counts(world, rows, koff, kref):
    """the pair counts (and "many": above 200) of the queries whose pairs are kept and dropped on both sides of n_primary"""
    out = set()
    for i, h in enumerate(rows):
        kept = set(kref[koff[i]:koff[i + 1]].tolist())
        sides = [[k in kept for k in h if k < world.n_primary], [k in kept for k in h if k >= world.n_primary]]
        if all(len(set(x)) == 2 for x in sides):
            out.add(len(h)); out |= {"many"} if len(h) > 200 else set()
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("annotate"))


def test_restated_rule_agrees_with_the_expected_values(world):
    """the arithmetic used for the expected values is annotate_restate.pair_value's"""
    q, rows = world.get(True)
    _, koff, kref, kval = world.expected(True, gtx.ANNOTATE_CENTER)
    refs = as_dicts(world.both, "x")
    want = [(k, ar.pair_value(refs[k], k >= world.n_primary, int(q["s"][i]), int(q["e"][i]), True)) for i, h in enumerate(rows) for k in h]
    assert [(k, v[2]) for k, v in want if v[0]] == list(zip(kref.tolist(), kval.tolist()))


@pytest.mark.parametrize("ign", [True, False], ids=["i", "strand"])
@pytest.mark.parametrize("mode", [gtx.ANNOTATE_CENTER, gtx.ANNOTATE_START], ids=["center", "start"])
def test_join_annotate_equals_the_restated_reference(engine, world, mode, ign):
    reads = world.load(engine, ign)
    rows, koff, kref, kval = world.expected(ign, mode)
    got_off, got_ref, got_val, n_pairs, info = engine.join_annotate(reads, world.n_primary, mode, gtx.JOIN_GAPS)
    assert n_pairs == sum(len(h) for h in rows) and info["n_no_class"] == 0
    assert np.array_equal(got_off, koff) and np.array_equal(got_ref, kref) and np.array_equal(got_val, kval)
    # the shapes the issue lists: every count around the threshold and a few hundred, each with kept and dropped pairs of both sets
    assert set(world.both["strand"]) == {0, 1} and len(rows) > 3000
    if mode == gtx.ANNOTATE_CENTER:
        assert mixed_counts(world, rows, koff, kref) >= set(COUNTS[2:]) | {"many"} and {len(h) for h in rows} >= set(COUNTS)
    else:
        assert np.array_equal(got_off, np.concatenate(([0], np.cumsum([len(h) for h in rows]))))
        assert got_ref.tolist() == [k for h in rows for k in h]


@pytest.mark.parametrize("which", ["none_primary", "all_primary"])
def test_n_primary_at_either_end(engine, world, which):
    reads = world.load(engine, True)
    n_primary = 0 if which == "none_primary" else len(world.both["s"])
    _, koff, kref, kval = world.expected(True, gtx.ANNOTATE_CENTER, n_primary=n_primary)
    got_off, got_ref, got_val, _, _ = engine.join_annotate(reads, n_primary, gtx.ANNOTATE_CENTER, gtx.JOIN_GAPS)
    assert np.array_equal(got_off, koff) and np.array_equal(got_ref, kref) and np.array_equal(got_val, kval)
    other = world.expected(True, gtx.ANNOTATE_CENTER)[3]
    assert not np.array_equal(kval, other)


def test_everything_dropped_and_everything_kept(engine):
    """50 '+' genes of 1000 bases 10 kb apart, no upstream set; a query [start - 10, start + 2] has offsets (-10, 2): dropped under
    center; a query [start + 5, start + 9] is kept"""
    starts = 5000 + 10_000 * np.arange(50)
    engine.set_refs(np.stack([np.zeros(50), starts, starts + 999], axis=1).astype(np.int32), 1)
    engine.set_ref_order(None); engine.set_ref_strands(None); engine.set_join_buffer(1 << 26)
    before = np.stack([np.zeros(50), starts - 10, starts + 2], axis=1).astype(np.int32)
    after = np.stack([np.zeros(50), starts + 5, starts + 9], axis=1).astype(np.int32)
    off, ref, val, n_pairs, _ = engine.join_annotate(before, 50, gtx.ANNOTATE_CENTER)
    assert n_pairs == 50 and not off.any() and len(ref) == 0 and len(val) == 0
    off, ref, val, n_pairs, _ = engine.join_annotate(after, 50, gtx.ANNOTATE_CENTER)
    assert n_pairs == 50 and np.array_equal(off, np.arange(51)) and np.array_equal(ref, np.arange(50)) and (val == 5 + 9).all()
    off, ref, val, _, _ = engine.join_annotate(before, 50, gtx.ANNOTATE_START)
    assert np.array_equal(off, np.arange(51)) and (val == -10).all()


def test_join_buffer_of_64_pairs_with_one_query_above_it(engine, world):
    reads = world.load(engine, True, buffer=64)
    rows, koff, kref, kval = world.expected(True, gtx.ANNOTATE_CENTER)
    assert max(len(h) for h in rows) > 64
    try:
        got_off, got_ref, got_val, n_pairs, _ = engine.join_annotate(reads, world.n_primary, gtx.ANNOTATE_CENTER, gtx.JOIN_GAPS)
    finally:
        engine.set_join_buffer(1 << 26)
    assert n_pairs == sum(len(h) for h in rows)
    assert np.array_equal(got_off, koff) and np.array_equal(got_ref, kref) and np.array_equal(got_val, kval)


def test_capacity_below_the_kept_count_then_the_repeat(engine, world):
    reads = world.load(engine, True)
    _, koff, kref, kval = world.expected(True, gtx.ANNOTATE_CENTER)
    cap = len(kref) // 3
    off, ref, val, _, _ = engine.join_annotate(reads, world.n_primary, gtx.ANNOTATE_CENTER, gtx.JOIN_GAPS, capacity=cap)
    assert np.array_equal(off, koff) and off[-1] > cap
    assert np.array_equal(ref, kref[:cap]) and np.array_equal(val, kval[:cap])
    off, ref, val, _, _ = engine.join_annotate(reads, world.n_primary, gtx.ANNOTATE_CENTER, gtx.JOIN_GAPS, capacity=int(off[-1]))
    assert np.array_equal(ref, kref) and np.array_equal(val, kval)


def device_pairs(engine, torch, reads):
    d_reads = torch.from_numpy(reads).cuda()
    n = len(reads)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    total, _, _ = engine.join_device(d_reads.data_ptr(), n, d_off.data_ptr(), 0, 0, gtx.JOIN_GAPS)
    d_pairs = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    tot, done, _ = engine.join_device(d_reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, gtx.JOIN_GAPS)
    assert tot == total and done == n
    return d_reads, d_off, d_pairs, total


def test_device_pass_and_its_capacity_contract(engine, world):
    torch = pytest.importorskip("torch")
    reads = world.load(engine, True)
    _, koff, kref, kval = world.expected(True, gtx.ANNOTATE_CENTER)
    d_reads, d_off, d_pairs, total = device_pairs(engine, torch, reads)
    n = len(reads)
    d_koff = torch.full((n + 1,), -3, dtype=torch.int64, device="cuda")
    cap = len(kref) // 2
    d_ref = torch.full((cap + 8,), -5, dtype=torch.int32, device="cuda")
    d_val = torch.full((cap + 8,), -5, dtype=torch.int64, device="cuda")
    kept = engine.pair_annotate_device(d_reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, world.n_primary, d_koff.data_ptr(),
                                       d_ref.data_ptr(), d_val.data_ptr(), cap, gtx.ANNOTATE_CENTER)
    assert kept == len(kref) and kept > cap
    assert np.array_equal(d_koff.cpu().numpy(), koff)
    assert np.array_equal(d_ref.cpu().numpy()[:cap], kref[:cap]) and np.array_equal(d_val.cpu().numpy()[:cap], kval[:cap])
    assert (d_ref.cpu().numpy()[cap:] == -5).all() and (d_val.cpu().numpy()[cap:] == -5).all()      # nothing behind the capacity
    d_ref = torch.zeros(kept, dtype=torch.int32, device="cuda"); d_val = torch.zeros(kept, dtype=torch.int64, device="cuda")
    again = engine.pair_annotate_device(d_reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, world.n_primary, d_koff.data_ptr(),
                                        d_ref.data_ptr(), d_val.data_ptr(), kept, gtx.ANNOTATE_CENTER)
    assert again == kept and np.array_equal(d_ref.cpu().numpy(), kref) and np.array_equal(d_val.cpu().numpy(), kval)


@pytest.mark.parametrize("op", ["5p", "3p"])
def test_start_mode_equals_the_offset_pass(engine, world, op):
    torch = pytest.importorskip("torch")
    reads = world.load(engine, True)
    d_reads, d_off, d_pairs, total = device_pairs(engine, torch, reads)
    n = len(reads)
    d_out = torch.zeros((total, 2), dtype=torch.int64, device="cuda")
    assert engine.pair_offsets_device(d_reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, d_out.data_ptr(), op) == -1
    d_koff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_ref = torch.zeros(total, dtype=torch.int32, device="cuda"); d_val = torch.zeros(total, dtype=torch.int64, device="cuda")
    kept = engine.pair_annotate_device(d_reads.data_ptr(), n, d_off.data_ptr(), d_pairs.data_ptr(), total, world.n_primary, d_koff.data_ptr(),
                                       d_ref.data_ptr(), d_val.data_ptr(), total, gtx.ANNOTATE_START, op, op)
    assert kept == total and total > 10_000
    assert torch.equal(d_koff, d_off) and torch.equal(d_ref, d_pairs) and torch.equal(d_val, d_out[:, 0])


def test_empty_query_set(engine, world):
    torch = pytest.importorskip("torch")
    world.load(engine, True)
    off, ref, val, n_pairs, _ = engine.join_annotate(np.zeros((0, 3), dtype=np.int32), world.n_primary)
    assert off.tolist() == [0] and len(ref) == 0 and len(val) == 0 and n_pairs == 0
    d_koff = torch.full((1,), -3, dtype=torch.int64, device="cuda")
    assert engine.pair_annotate_device(0, 0, 0, 0, 0, world.n_primary, d_koff.data_ptr(), 0, 0, 0) == 0
    assert d_koff.cpu().tolist() == [0]


def test_bad_arguments_are_errors(engine, world):
    reads = world.load(engine, True)
    for kw in (dict(mode=0), dict(mode=3), dict(op_primary="5p", op_rest="3p", n_primary=-1), dict(n_primary=len(world.both["s"]) + 1)):
        with pytest.raises(gtx.GtxError):
            engine.join_annotate(reads[:10], kw.pop("n_primary", world.n_primary), **kw)
