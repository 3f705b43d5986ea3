"""The line renderer on the device (gtx_lines_layout, gtx_window_lines_device, gtx_pair_lines_device and the streaming host entries)
against its restatement (tests/window_lines_cases.py: render, render_pairs), byte for byte, on synthetic vectors made with torch.  The
text buffer is filled with a sentinel first: behind the bytes a call reports, from the next 16-byte boundary on, and in a guard behind
the capacity, every byte must still be the sentinel."""
import numpy as np
import pytest
import torch

import gtx
import window_lines_cases as W

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 256
CASES = W.all_cases()
PAIRS = W.pair_cases()


@pytest.fixture(scope="module")
def expected():
    """every case's text, lines and end, rendered once"""
    want = {c["name"]: W.render(c["values"], c["layout"], c["min_value"], c["limit"], c["first"], c["count"]) for c in CASES}
    want.update({c["name"]: W.render_pairs(c["ordinals"], c["values"], c["layout"], c["limit"], c["first"], c["count"]) for c in PAIRS})
    return want


def on_device(a):
    if isinstance(a, W.SparseVec):
        t = torch.zeros(len(a), dtype=torch.int64, device="cuda")
        t[a.start:a.start + len(a.part)] = torch.from_numpy(a.part.view(np.int64)).cuda()
        return t
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    return t if len(t) else torch.zeros(2, dtype=torch.int64, device="cuda")


def layout_on(engine, lay):
    mb = engine.lines_layout(lay.block_offset, lay.names, lay.strands, lay.step, lay.size)
    assert mb == lay.max_bytes()
    return mb


def text_buffer(capacity):
    return torch.full((capacity + GUARD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")


def check_text(buf, capacity, got, want):
    n_lines, n_bytes, end_at = got
    out = buf.cpu().numpy()
    assert out[:n_bytes].tobytes() == want[0]
    assert (n_lines, end_at) == (want[1], want[2]) and n_bytes == len(want[0]) <= capacity
    assert np.all(out[(n_bytes + 15) // 16 * 16:] == SENTINEL)                  # nothing behind the unit the text ends in, nothing behind the capacity


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_window_lines_device(engine, expected, c):
    mb = layout_on(engine, c["layout"])
    d_v = on_device(c["values"])
    capacity = c["count"] * mb                                                  # an exact fit of the bound
    buf = text_buffer(capacity)
    got = engine.window_lines_device(d_v.data_ptr(), c["first"], c["count"], c["limit"], c["min_value"], buf.data_ptr(), capacity)
    check_text(buf, capacity, got, expected[c["name"]])


@pytest.mark.parametrize("c", PAIRS, ids=[c["name"] for c in PAIRS])
def test_pair_lines_device(engine, expected, c):
    mb = layout_on(engine, c["layout"])
    d_o, d_v = on_device(c["ordinals"]), on_device(c["values"])
    capacity = c["count"] * mb
    buf = text_buffer(capacity)
    got = engine.pair_lines_device(d_o.data_ptr(), d_v.data_ptr(), c["first"], c["count"], c["limit"], buf.data_ptr(), capacity)
    check_text(buf, capacity, got, expected[c["name"]])


def test_value_two_to_the_63_by_rule(engine):
    """negative as signed: printed under a negative min_value, dropped under 0, dropped by the pair rule"""
    lay = W.one_block(4)
    mb = layout_on(engine, lay)
    v = np.array([5, 1 << 63, 6, 7], dtype=np.uint64)
    d_v, d_o = on_device(v), on_device(np.arange(4, dtype=np.int64))
    buf = text_buffer(4 * mb)
    got = engine.window_lines_device(d_v.data_ptr(), 0, 4, 4, -(1 << 63), buf.data_ptr(), 4 * mb)
    assert got[0] == 4 and b"\n-9223372036854775808\tchr1 + 26 525\n" in buf.cpu().numpy()[:got[1]].tobytes()
    assert engine.window_lines_device(d_v.data_ptr(), 0, 4, 4, 0, buf.data_ptr(), 4 * mb)[0] == 3
    assert engine.pair_lines_device(d_o.data_ptr(), d_v.data_ptr(), 0, 4, 4, buf.data_ptr(), 4 * mb)[0] == 3
    assert b"-" not in buf.cpu().numpy()[:engine.pair_lines_device(d_o.data_ptr(), d_v.data_ptr(), 0, 4, 4, buf.data_ptr(), 4 * mb)[1]].tobytes()


def test_a_name_above_the_limit_is_refused(engine):
    ok = W.Layout([0, 10], ["n" * W.MAX_NAME], "+", 25, 500)
    layout_on(engine, ok)
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        engine.lines_layout([0, 10], ["n" * (W.MAX_NAME + 1)], "+", 25, 500)
    with pytest.raises(gtx.GtxError, match="gtx error -3"):                     # a refused layout is no layout
        engine.lines_max_bytes()
    for bad in (dict(block_offset=[0, 10, 5], names=["a", "b"], strands="++"), dict(block_offset=[1, 10], names=["a"], strands="+"),
                dict(block_offset=[0, 10], names=["a"], strands="*")):
        with pytest.raises(gtx.GtxError, match="gtx error -1"):
            engine.lines_layout(bad["block_offset"], bad["names"], bad["strands"], 25, 500)


def test_capacity_one_byte_under_the_bound_writes_nothing(engine):
    lay = W.one_block(W.TILE + 9)
    mb = layout_on(engine, lay)
    n = lay.total
    d_v = on_device(np.full(n, 12, dtype=np.uint64))
    buf = text_buffer(n * mb)
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        engine.window_lines_device(d_v.data_ptr(), 0, n, n, 0, buf.data_ptr(), n * mb - 1)
    with pytest.raises(gtx.GtxError, match="gtx error -1"):
        engine.pair_lines_device(d_v.data_ptr(), d_v.data_ptr(), 0, n, n, buf.data_ptr(), n * mb - 1)
    with pytest.raises(gtx.GtxError, match="gtx error -1"):                     # a range beyond the layout's windows
        engine.window_lines_device(d_v.data_ptr(), 1, n, n, 0, buf.data_ptr(), n * mb)
    with pytest.raises(gtx.GtxError, match="gtx error -1"):                     # an unaligned text buffer
        engine.window_lines_device(d_v.data_ptr(), 0, n, n, 0, buf.data_ptr() + 8, n * mb)
    assert bool(torch.all(buf == SENTINEL))
    got = engine.window_lines_device(d_v.data_ptr(), 0, n, n, 0, buf.data_ptr(), n * mb)
    check_text(buf, n * mb, got, W.render(np.full(n, 12, dtype=np.uint64), lay, 0, n))


# ---- the streaming host entries ----
@pytest.fixture()
def small_chunks(engine):
    """a chunk of one tile's bound: a few thousand windows make tens of chunks"""
    def setter(lay):
        layout_on(engine, lay)
        engine.set_lines_chunk(W.chunk_bound(lay))
    yield setter
    engine.set_lines_chunk(64 << 20)


def stream_case():
    rng = np.random.default_rng(29)
    lay = W.stranded([9 * W.TILE + 300, 6 * W.TILE + 5, 40], ["chr1", "chr2", "chrX"])
    v = rng.integers(0, 40, lay.total).astype(np.uint64)
    v[3 * W.TILE:4 * W.TILE] = 0                                                 # a range without a line: no call of the sink for it
    return lay, v


def test_window_lines_streams_whole_tiles_in_order(engine, small_chunks):
    lay, v = stream_case()
    small_chunks(lay)
    d_v = on_device(v)
    chunks, n_lines, n_bytes, end_at = engine.window_lines(d_v.data_ptr(), lay.total, 10, n_windows=lay.total)
    want = [W.render(v, lay, 10, lay.total, f, min(W.TILE, lay.total - f))[0] for f in range(0, lay.total, W.TILE)]
    assert chunks == [t for t in want if t] and len(chunks) == len(want) - 1 >= 30    # cut at tile ends: no line straddles two chunks
    whole = W.render(v, lay, 10, lay.total)
    assert b"".join(chunks) == whole[0] and (n_lines, n_bytes, end_at) == (whole[1], len(whole[0]), -1)
    # a larger chunk, a limit, an all-ones value: the stream ends there
    engine.set_lines_chunk(3 * W.chunk_bound(lay) + 17)
    v[5 * W.TILE + 77] = W.ONES
    d_v = on_device(v)
    for limit in (lay.total, 5 * W.TILE + 77, 2 * W.TILE + 1):
        chunks, n_lines, n_bytes, end_at = engine.window_lines(d_v.data_ptr(), limit, 10, n_windows=lay.total)
        whole = W.render(v, lay, 10, limit)
        assert b"".join(chunks) == whole[0] and (n_lines, n_bytes, end_at) == (whole[1], len(whole[0]), whole[2])
        assert all(len(t) <= 3 * W.chunk_bound(lay) for t in chunks)
    assert W.render(v, lay, 10, lay.total)[2] == 5 * W.TILE + 77


def test_a_sink_that_refuses_ends_the_call(engine, small_chunks):
    lay, v = stream_case()
    small_chunks(lay)
    d_v = on_device(v)
    calls = []

    def sink(text):
        calls.append(text)
        return len(calls) == 3

    with pytest.raises(gtx.GtxError, match="gtx error %d" % gtx.E_SINK):
        engine.window_lines(d_v.data_ptr(), lay.total, 10, n_windows=lay.total, sink=sink)
    assert len(calls) == 3 and b"".join(calls) == W.render(v, lay, 10, lay.total, 0, 3 * W.TILE)[0]
    # the context goes on working
    chunks, n_lines, _, _ = engine.window_lines(d_v.data_ptr(), lay.total, 10, n_windows=lay.total)
    assert b"".join(chunks) == W.render(v, lay, 10, lay.total)[0]


def test_pair_lines_streams(engine, small_chunks):
    c = next(p for p in PAIRS if p["name"] == "gaps of many tiles")
    lay = c["layout"]
    small_chunks(lay)
    d_o, d_v = on_device(c["ordinals"]), on_device(c["values"])
    n = len(c["ordinals"])
    chunks, n_lines, n_bytes, end_at = engine.pair_lines(d_o.data_ptr(), d_v.data_ptr(), n, lay.total)
    want = [W.render_pairs(c["ordinals"], c["values"], lay, lay.total, f, min(W.TILE, n - f))[0] for f in range(0, n, W.TILE)]
    assert chunks == want and len(chunks) == 3
    assert (n_lines, n_bytes, end_at) == (n, sum(len(t) for t in want), -1)


def test_filter_lines_is_the_filter_then_the_pair_rule(engine, small_chunks):
    rng = np.random.default_rng(31)
    lengths, step, size = [60000, 21000], 25, 500
    nw = [gtx.load().gtx_scan_n_windows(ln, step, size) for ln in lengths]
    lay = W.Layout([0, nw[0], nw[0] + nw[1]], ["chr1", "chr2"], "++", step, size)
    small_chunks(lay)
    v = rng.integers(0, 30, lay.total).astype(np.uint64)
    refs = np.array([[0, 1000, 9000], [0, 30000, 30010], [1, 1, 700], [1, 20000, 25000]], dtype=np.int32)
    engine.window_refs(refs, lengths, [0, nw[0]], step, size)
    d_v = on_device(v)
    ordinals, values, kept = engine.window_filter(d_v.data_ptr(), min_value=12, n_windows=lay.total)
    assert 100 < kept < lay.total // 2
    for limit in (lay.total, int(ordinals[kept // 2])):
        chunks, n_lines, n_bytes, end_at = engine.window_filter_lines(d_v.data_ptr(), 12, limit, n_windows=lay.total)
        whole = W.render_pairs(ordinals, values, lay, limit)
        assert b"".join(chunks) == whole[0] and (n_lines, end_at) == (whole[1], -1) and n_lines > 0
