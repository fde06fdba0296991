"""lsdr_ts_stitch on the GPU against the numpy restatement of its definition (stitch_common): joins, kept ranges and the output's bytes,
bit for bit.  Streams cut from ts_common.build_stream(n=3000), P = 4, W = 256, M = 8, max_packets = 1200 (stitch_common.cases)."""

import numpy as np
import pytest
import stitch_common as sc

pytestmark = pytest.mark.gpu

CASES = sc.cases()


@pytest.fixture(scope="module")
def wanted():
    """The restatement's (joins, keep, bytes) of every case, once."""
    return [sc.stitch(streams) for _, streams, _ in CASES]


class Uploaded:
    """Streams in device memory: pointers (None for an empty one) and lengths."""

    def __init__(self, ctx, streams):
        self.bufs = [ctx.upload(np.ascontiguousarray(s)) if len(s) else None for s in streams]
        self.ptrs = [b.ptr if b else None for b in self.bufs]
        self.n = [len(s) for s in streams]

    def free(self):
        for b in self.bufs:
            if b:
                b.free()


def run(capi, ctx, obj, streams):
    up = Uploaded(ctx, streams)
    try:
        return obj.stitch(up.ptrs, up.n)
    finally:
        up.free()


@pytest.fixture(scope="module")
def stitcher(capi, ctx):
    obj = capi.TsStitch(ctx, 4, sc.MAX_PACKETS, window=sc.W, min_run=sc.M)
    yield obj
    obj.close()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_equals_the_restatement(capi, ctx, stitcher, wanted, k):
    name, streams, joined = CASES[k]
    joins, keep, ts = run(capi, ctx, stitcher, streams)                   # (one object for all cases: reused)
    print(name, joins, keep)
    assert joins == wanted[k][0], name
    assert keep == wanted[k][1], name
    assert ts == wanted[k][2], name
    assert [j["joined"] for j in joins] == joined, name


def test_equal_keys_are_told_apart_by_the_bytes(capi, ctx, wanted, monkeypatch):
    """With the key function a constant (LSDR_TS_STITCH_CONST_KEY, read at create) every pair of packets that are not null meets with
    equal keys; the byte compare alone decides, and the records are the same."""
    monkeypatch.setenv("LSDR_TS_STITCH_CONST_KEY", "1")
    obj = capi.TsStitch(ctx, 4, sc.MAX_PACKETS, window=sc.W, min_run=sc.M)
    monkeypatch.delenv("LSDR_TS_STITCH_CONST_KEY")
    try:
        for k, (name, streams, _) in enumerate(CASES):
            assert run(capi, ctx, obj, streams) == wanted[k], name
        # two packets that differ in their last byte only, at the same place of an otherwise equal overlap
        b = sc.base()
        a0, a1 = b[0:900].copy(), b[800:1700].copy()
        a1[30, 187] ^= 0x80
        streams = [a0, a1, b[1600:2400], b[2300:]]
        got = run(capi, ctx, obj, streams)
        assert got == sc.stitch(streams) and got[0][0]["run"] == 69
    finally:
        obj.close()


def test_alone_at_any_position_and_on_a_reused_object(capi, ctx, stitcher, wanted):
    name, streams, _ = CASES[3]                                           # deleted on both sides
    pair = capi.TsStitch(ctx, 2, sc.MAX_PACKETS, window=sc.W, min_run=sc.M)
    six = capi.TsStitch(ctx, 6, sc.MAX_PACKETS, window=sc.W, min_run=sc.M)
    try:
        for k in range(3):                                                # every pair alone
            joins, keep, ts = run(capi, ctx, pair, streams[k:k + 2])
            assert joins == [wanted[3][0][k]] and (joins, keep, ts) == sc.stitch(streams[k:k + 2])
        other = CASES[5][1]
        for lead in ([], [other[0]], [other[0], other[1]]):               # the same four streams behind zero, one and two others
            batch = lead + streams + other[:2 - len(lead)]
            joins, keep, ts = run(capi, ctx, six, batch)
            assert (joins, keep, ts) == sc.stitch(batch)
            assert joins[len(lead):len(lead) + 3] == wanted[3][0]
        # a reused object: another case in between, then the same records again
        first = run(capi, ctx, stitcher, streams)
        run(capi, ctx, stitcher, CASES[4][1])
        assert run(capi, ctx, stitcher, streams) == first == wanted[3]
    finally:
        pair.close()
        six.close()


def test_unaligned_pointers_and_one_stream(capi, ctx):
    """Streams at 4-byte aligned addresses that are not 16-byte aligned (the key pass and the gather take their other paths), and P = 1."""
    b = sc.base()
    streams = [b[0:900], b[800:1700], b[1600:2400], b[2300:]]
    obj = capi.TsStitch(ctx, 4, sc.MAX_PACKETS, window=sc.W, min_run=sc.M)
    one = capi.TsStitch(ctx, 1, sc.MAX_PACKETS, window=sc.W, min_run=sc.M)
    bufs = [ctx.upload(np.concatenate([np.zeros(4 * (k + 1), np.uint8), s.reshape(-1)])) for k, s in enumerate(streams)]
    try:
        got = obj.stitch([buf.ptr + 4 * (k + 1) for k, buf in enumerate(bufs)], [len(s) for s in streams])
        assert got == sc.stitch(streams)
        assert one.stitch([bufs[2].ptr + 12], [len(streams[2])]) == sc.stitch([streams[2]])
        assert one.stitch([None], [0]) == ([], [dict(start=0, end=0, out_offset=0)], b"")
    finally:
        for buf in bufs:
            buf.free()
        obj.close()
        one.close()


@pytest.mark.parametrize("const_key", [0, 1])
def test_runs_longer_than_a_chunk(capi, ctx, monkeypatch, const_key):
    """W = 1024: overlaps of 700 and 600 packets, whose runs cross the 256 cells a workgroup verifies at a time and the 512 rows the span
    pass stages at a time — whole, and cut in two by a packet deleted on either side; with the constant key every diagonal is verified."""
    b = sc.base()
    whole = [b[0:1500], b[800:2300], b[1700:]]
    cut = [b[0:1500], np.delete(b[800:2300], [300, 1000], axis=0), np.delete(b[1700:], [256], axis=0)]
    monkeypatch.setenv("LSDR_TS_STITCH_CONST_KEY", str(const_key))
    obj = capi.TsStitch(ctx, 3, 1500, window=1024, min_run=8)
    try:
        for streams in (whole, cut):
            got, want = run(capi, ctx, obj, streams), sc.stitch(streams, 1024, 8)
            print([j["run"] for j in want[0]])
            assert got == want
        assert [j["run"] for j in sc.stitch(whole, 1024, 8)[0]] == [700, 600]
    finally:
        obj.close()


def test_refusals(capi, ctx, stitcher):
    with pytest.raises(capi.LsdrError, match="ts_stitch"):
        capi.TsStitch(ctx, 0, 100)
    with pytest.raises(capi.LsdrError, match="ts_stitch"):
        capi.TsStitch(ctx, 2, 100, window=70000)
    with pytest.raises(capi.LsdrError, match="ts_stitch"):
        capi.TsStitch(ctx, 2, 100, window=16, min_run=17)
    buf = ctx.upload(np.zeros(16 * 188, np.uint8))
    try:
        with pytest.raises(capi.LsdrError, match="max_packets"):
            stitcher.run_async([buf.ptr, None, None, None], [sc.MAX_PACKETS + 1, 0, 0, 0])
        with pytest.raises(capi.LsdrError, match="no pointer"):
            stitcher.run_async([None, None, None, None], [1, 0, 0, 0])
        with pytest.raises(capi.LsdrError, match="aligned"):
            stitcher.run_async([buf.ptr + 2, None, None, None], [1, 0, 0, 0])
        with pytest.raises(capi.LsdrError, match="no run in flight"):
            stitcher.wait()
        stitcher.run_async([buf.ptr, None, None, None], [16, 0, 0, 0])
        with pytest.raises(capi.LsdrError, match="in flight"):
            stitcher.run_async([buf.ptr, None, None, None], [16, 0, 0, 0])
        joins, keep = stitcher.wait()
        assert keep[0] == dict(start=0, end=16, out_offset=0) and stitcher.download() == bytes(16 * 188)
    finally:
        buf.free()
