"""lsdr_ts_batch on the GPU: the census and the PID filter of many transport streams in device memory.

  a census against the restatement: summary and table equal ts_common.census bit for bit — the builder's 3000-packet stream with its
    injected events, leantsgen's pattern (5000 packets; 70000 packets with a table of 64 and of 8192), and 2000 packets of uniformly
    random bytes with the sync byte in nine of ten (every field arbitrary, many PIDs with one packet) — at the default tile and at
    the smallest one (LSDR_TS_BATCH_TILE=256);
  b tile seams: lengths 0, 1, T − 1, T, T + 1, 2T + 3; a PID whose consecutive packets lie in tiles 0 and 2 with none in tile 1 and an
    error exactly on that pair; a PCR PID whose first and last PCR sit in the first and the last tile (and a second PID with PCRs that
    starts later and is not the PCR PID);
  c a stream alone equals the same stream in a ragged batch of five that contains a stream of no packets with a NULL pointer;
  d the filter: bytes, kept and index equal the numpy selection for per-stream PID lists, every drop combination, nothing kept and
    everything kept (the output is the input); download_async delivers out_dev's bytes, a buffer one byte too small is refused, a
    pending download survives the next run_async;
  e every refusal is LSDR_E_ARG (LSDR_E_UNSUPPORTED for max_packets ≥ 2^32) with a message naming ts_batch and leaves a usable object;
  f end to end: the builder's 600-packet multi-PID stream WITHOUT injected events (the test asserts that the decoders lose nothing of
    it; a stream with deleted packets has continuity errors of its own) through synth_dvbs.modulate at 1.2 samples per symbol, quantised
    as capture_u8 does (amplitude 75, noise 7.5; 979200 symbols, 1.17 M samples), and a twin with six_variants' garbage burst (200000
    samples, see BURST) in the middle, through CaptureBatch (default and Viterbi) and HsBatch: ts_census equals the restatement on the TS that decode returned, the
    clean capture has no continuity error behind bench_c1.SKIP_ACQ packets, the twin has cc_missing > 0, and ts_filter on one PID
    returns exactly that PID's packets.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import ts_common as tc
from leansdr_amd import synth_dvbs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _stream(name):
    if name == "built":
        return tc.build_stream(3000)[0]
    if name == "random":
        rng = np.random.default_rng(33)
        pk = rng.integers(0, 256, (2000, 188)).astype(np.uint8)
        pk[rng.random(2000) < 0.9, 0] = 0x47
        return pk
    return synth_dvbs.ts_packets(int(name))


@functools.lru_cache(maxsize=None)
def _want(name, n=None, max_pids=64):
    return tc.census(_stream(name)[:n], max_pids)


def _make(capi, ctx, n_streams, max_packets, max_pids=64, tile=None):
    old = os.environ.pop("LSDR_TS_BATCH_TILE", None)
    if tile:
        os.environ["LSDR_TS_BATCH_TILE"] = str(tile)
    try:
        tb = capi.TsBatch(ctx, n_streams, max_packets, max_pids)
    finally:
        os.environ.pop("LSDR_TS_BATCH_TILE", None)
        if old is not None:
            os.environ["LSDR_TS_BATCH_TILE"] = old
    assert tb.tile == (tile or 1024)
    return tb


class _Uploaded:
    """Streams (uint8 [N][188], or None for no packets and a NULL pointer) in device memory."""

    def __init__(self, ctx, streams):
        self.bufs = [ctx.upload(s) if s is not None and len(s) else None for s in streams]
        self.ptrs = [b.ptr if b else None for b in self.bufs]
        self.n = [len(s) if s is not None else 0 for s in streams]

    def free(self):
        for b in self.bufs:
            if b:
                b.free()


def _census(capi, ctx, streams, max_pids=64, tile=None):
    up = _Uploaded(ctx, streams)
    tb = _make(capi, ctx, len(streams), max(up.n + [1]), max_pids, tile)
    try:
        return tb.census(up.ptrs, up.n)
    finally:
        tb.close()
        up.free()


# ---- a -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [None, 256])
def test_census_equals_the_restatement(capi, ctx, tile):
    names = ["built", "5000", "70000", "random"]
    got = _census(capi, ctx, [_stream(k) for k in names], 64, tile)
    for k, g in zip(names, got):
        w = _want(k)
        assert g == w, f"{k}:\n device {({a: b for a, b in g.items() if a != 'pids'})}\n wanted {({a: b for a, b in w.items() if a != 'pids'})}"
    wide = _census(capi, ctx, [_stream("70000"), _stream("random")], 8192, tile)
    assert wide[0] == _want("70000", None, 8192) and wide[1] == _want("random", None, 8192)
    # the inputs are what they are meant to be
    assert got[2]["pids_seen"] == 274 and got[2]["pids_listed"] == 64 and wide[0]["pids_listed"] == 274
    assert got[3]["pids_seen"] > 500 and got[3]["sync_errors"] > 100 and got[3]["tei"] > 500 and got[3]["pcr_count"] >= 1
    assert got[3]["cc_errors"] > 0 and got[3]["discontinuities"] > 0 and got[3]["pids_seen"] < got[3]["valid"]
    assert got[0]["cc_repeats"] == 3 and got[0]["discontinuities"] == 1 and got[0]["cc_missing"] == 5


# ---- b -----------------------------------------------------------------------------------------------------------------------------
def _packet(pid, cc, afc=1, pcr=None):
    p = np.full(188, 0xff, np.uint8)
    p[0], p[1], p[2], p[3] = 0x47, pid >> 8, pid & 255, (afc << 4) | (cc & 15)
    if afc & 2:
        p[4], p[5] = 183 if afc == 2 else 7, 0
    if pcr is not None:
        p[4], p[5] = 7, 0x10
        p[6:12] = tc.pcr_bytes(pcr)
    return p


def _seam_stream(T):
    """3T packets of PID 0x20 with a correct counter, except: PID 0x21 at T − 3 (cc 3) and at 2T + 2 (cc 9: expected 4, one error, missing
    5) and nowhere in tile 1; PID 0x30 with PCRs at 2 and 3T − 2; PID 0x31 with PCRs at T + 1 and 2T − 1."""
    pk = np.stack([_packet(0x20, k) for k in range(3 * T)])
    pk[T - 3], pk[2 * T + 2] = _packet(0x21, 3), _packet(0x21, 9)
    pk[2], pk[3 * T - 2] = _packet(0x30, 0, 2, 27_000_000), _packet(0x30, 0, 2, 27_000_000 + 4000 * (3 * T - 4))
    pk[T + 1], pk[2 * T - 1] = _packet(0x31, 7, 3, 5), _packet(0x31, 8, 3, 6)
    return pk


@pytest.mark.parametrize("tile", [None, 256])
def test_tile_seams(capi, ctx, tile):
    T = tile or 1024
    built = _stream("built")
    lengths = [0, 1, T - 1, T, T + 1, 2 * T + 3]
    assert lengths[-1] <= len(built)
    seam = _seam_stream(T)
    got = _census(capi, ctx, [built[:n] if n else None for n in lengths] + [seam], 64, tile)
    for n, g in zip(lengths, got):
        assert g == _want("built", n), f"{n} packets"
    assert got[0]["pids_seen"] == 0 and got[0]["pcr_pid"] == -1 and got[0]["pids"] == []
    g = got[-1]
    assert g == tc.census(seam)
    by_pid = {p["pid"]: p for p in g["pids"]}
    assert (by_pid[0x21]["cc_errors"], by_pid[0x21]["cc_missing"], by_pid[0x21]["first_packet"], by_pid[0x21]["last_packet"]) == (1, 5, T - 3, 2 * T + 2)
    assert (g["pcr_pid"], g["pcr_count"], g["pcr_first_packet"], g["pcr_last_packet"]) == (0x30, 2, 2, 3 * T - 2)
    assert (g["pcr_first"], g["pcr_last"]) == (27_000_000, 27_000_000 + 4000 * (3 * T - 4)) and by_pid[0x31]["pcr_count"] == 2
    assert capi.ts_bitrate(g) == 188 * 8 * 27e6 / 4000


# ---- c -----------------------------------------------------------------------------------------------------------------------------
def test_alone_and_in_a_ragged_batch(capi, ctx):
    streams = [_stream("built")[:1500], _stream("5000"), None, _stream("random"), _stream("built")]
    want = [tc.census(s if s is not None else np.zeros((0, 188), np.uint8)) for s in streams]
    got = _census(capi, ctx, streams)
    assert got == want
    up = _Uploaded(ctx, streams)
    one = _make(capi, ctx, 1, 5000)
    try:
        for i in range(len(streams)):
            assert one.census([up.ptrs[i]], [up.n[i]]) == [want[i]], i
    finally:
        one.close()
        up.free()


# ---- d -----------------------------------------------------------------------------------------------------------------------------
def _filter_streams():
    return [_stream("built"), _stream("random"), _stream("5000")[:1300], None]


def _selection(streams, keep, drops):
    per = [keep] * len(streams) if keep is None or not keep or np.isscalar(keep[0]) else keep
    out = []
    for s, k in zip(streams, per):
        s = s if s is not None else np.zeros((0, 188), np.uint8)
        idx = tc.kept(s, k, *drops)
        out.append((tc.select(s, idx), idx.astype(np.uint32)))
    return out


def test_filter_equals_the_numpy_selection(capi, ctx):
    streams = _filter_streams()
    some = sorted(set(tc.fields(streams[1])["pid"][:40].tolist()))
    rules = [([[tc.VIDEO], some, [0, 3], [5]], (True, True, True)), ([], (True, True, True)), (None, (False, False, False))]
    rules += [(keep, (a, b, c)) for keep in (None, [tc.AUDIO, tc.NULL_PID, 2] + some) for a in (False, True) for b in (False, True) for c in (False, True)]
    up = _Uploaded(ctx, streams)
    tb = _make(capi, ctx, len(streams), 3000)
    try:
        census = tb.census(up.ptrs, up.n)
        assert all(s["kept"] == 0 for s in census)
        for keep, drops in rules:
            res, data, idx = tb.filter(up.ptrs, up.n, keep, *drops, index=True)
            for i, ((wb, wi), s) in enumerate(zip(_selection(streams, keep, drops), res)):
                assert s["kept"] == len(wi) and data[i] == wb and np.array_equal(idx[i], wi), (keep, drops, i, s["kept"], len(wi))
                assert {k: v for k, v in s.items() if k != "kept"} == {k: v for k, v in census[i].items() if k != "kept"}
        # everything kept: the output is the input
        res, data, idx = tb.filter(up.ptrs, up.n, None, False, False, False)
        assert idx is None and all(data[i] == (streams[i].tobytes() if streams[i] is not None else b"") for i in range(len(streams)))
        assert [s["kept"] for s in res] == up.n and tb.index_ptr(0) is None
    finally:
        tb.close()
        up.free()


def test_download_of_the_kept_packets(capi, ctx):
    streams = _filter_streams()
    up = _Uploaded(ctx, streams)
    tb = _make(capi, ctx, len(streams), 3000)
    try:
        want_a = [b for b, _ in _selection(streams, [tc.VIDEO, 7], (True, True, True))]
        want_b = [b for b, _ in _selection(streams, None, (True, False, False))]
        rule_a, keep_a = tb.rule([tc.VIDEO, 7])
        tb.run_async(up.ptrs, up.n, rule_a)
        res = tb.wait()
        assert [s["kept"] * 188 for s in res] == [len(b) for b in want_a] and max(s["kept"] for s in res) > 1000
        cap = max(len(b) for b in want_a)
        bufs = [np.zeros(cap, np.uint8) for _ in streams]
        with pytest.raises(capi.LsdrError, match="ts_batch"):
            tb.download_async(bufs, cap - 1)                              # one byte too small
        # what lies at out_dev is what the download delivers
        direct = [np.empty(len(b), np.uint8) for b in want_a]
        for i, a in enumerate(direct):
            if len(a):
                capi.check(capi.lib.lsdr_memcpy_d2h(ctx.h, a.ctypes.data, tb.out_ptr(i), a.nbytes))
        ctx.sync()
        assert [a.tobytes() for a in direct] == want_a and tb.out_ptr(len(streams)) is None
        # a pending download survives the next run_async, which writes other packets to the same buffers
        tb.download_async(bufs, cap)
        rule_b, _ = tb.rule(None, True, False, False)
        tb.run_async(up.ptrs, up.n, rule_b)
        res_b = tb.wait()
        tb.download_wait()
        assert [bufs[i][:len(want_a[i])].tobytes() for i in range(len(streams))] == want_a
        assert [s["kept"] * 188 for s in res_b] == [len(b) for b in want_b]
        big = [np.zeros(max(len(b) for b in want_b), np.uint8) for _ in streams]
        tb.download_async(big)
        tb.download_wait()
        assert [big[i][:len(want_b[i])].tobytes() for i in range(len(streams))] == want_b
        tb.download_wait()                                                # nothing pending: returns at once
    finally:
        tb.close()
        up.free()


# ---- e -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_object_usable(capi, ctx):
    def refused(rc_want, **kw):
        cfg = capi.TsBatchCfg()
        cfg.n_streams, cfg.max_packets, cfg.max_pids = kw.get("n_streams", 2), kw.get("max_packets", 4096), kw.get("max_pids", 0)
        cfg.reserved[5] = kw.get("reserved", 0)
        h = C.c_void_p()
        rc = capi.lib.lsdr_ts_batch_create(ctx.h, C.byref(cfg), C.byref(h))
        assert rc == rc_want and not h and b"ts_batch" in capi.lib.lsdr_last_error(), (kw, rc, capi.lib.lsdr_last_error())
    refused(-2, n_streams=0); refused(-2, n_streams=-1); refused(-2, max_pids=8193); refused(-2, reserved=1)
    refused(-4, max_packets=1 << 32)

    built = _stream("built")
    want = _want("built", 2000)
    buf = ctx.upload(built)
    tb = _make(capi, ctx, 2, 2000, 8192)
    try:
        def fails(call):
            with pytest.raises(capi.LsdrError, match="ts_batch"):
                call()
        host = [np.zeros(2000 * 188, np.uint8) for _ in range(2)]
        fails(tb.wait)                                                                         # nothing in flight
        fails(lambda: tb.download_async(host))                                                 # no run with a rule yet
        fails(lambda: tb.run_async([buf.ptr, None], [2001, 0]))                                # more than max_packets
        fails(lambda: tb.run_async([buf.ptr, None], [100, 1]))                                 # packets without a pointer
        fails(lambda: tb.run_async([buf.at(2), None], [100, 0]))                               # not 4-byte aligned
        bad, _ = tb.rule()
        bad.drop = 8
        fails(lambda: tb.run_async([buf.ptr, None], [100, 0], bad))                            # unknown drop bits
        bad, _ = tb.rule()
        bad.reserved[0] = 1
        fails(lambda: tb.run_async([buf.ptr, None], [100, 0], bad))
        fails(tb.wait)                                                                         # … and nothing was queued
        tb.run_async([buf.ptr, None], [2000, 0])
        fails(lambda: tb.run_async([buf.ptr, None], [2000, 0]))                                # a run in flight
        got = tb.wait()
        assert got[0] == want and got[1]["packets"] == 0 and got[1]["pids"] == []
        fails(tb.wait)
        fails(lambda: tb.download_async(host))                                                 # the last run had no rule
        n = C.c_uint()
        for i in (-1, 2):
            assert capi.lib.lsdr_ts_batch_pids(tb.h, i, tb._tab, 8192, C.byref(n)) == -2 and b"ts_batch" in capi.lib.lsdr_last_error()
        assert capi.lib.lsdr_ts_batch_pids(tb.h, 0, tb._tab, 2, C.byref(n)) == -2 and n.value == 5   # a table too small: refused, told how many
        ok, _ = tb.rule()
        tb.run_async([buf.ptr, buf.at(188 * 4)], [2000, 1000], ok)
        fails(lambda: tb.download_async(host))                                                 # not waited for yet
        res = tb.wait()
        assert [r["kept"] for r in res] == [len(tc.kept(built[:2000])), len(tc.kept(built[4:1004]))]
        assert tb.census([buf.ptr, buf.ptr], [2000, 2000]) == [want, want]
    finally:
        tb.close()
        buf.free()


# ---- f -----------------------------------------------------------------------------------------------------------------------------
# The burst has to cost packets AND leave every engine locked again inside the half capture behind it: a loss shows as a counter jump only
# if packets follow it.  Measured on an MI355X on this capture (packets returned; clean 546 / 532 / 556 for default / Viterbi / hs): the
# Viterbi and hs engines come back after every burst tried (2000 … 200000 samples: 520 … 357 and 541 … 413 packets, cc_missing 8 … 27);
# the default engine comes back after 2000 samples (534) and after 200000 (419, cc_missing 28) but after 5000, 20000, 50000 and 100000
# samples it ends unlocked with the 247 packets in front of the burst — nothing follows the loss, and the census of such a TS rightly
# shows no jump.  (The reference binary's default graph returns 354 … 482 packets for those four.)  So: 200000 samples.
BURST = 200000

@functools.lru_cache(maxsize=None)
def _captures():
    """(the clean capture, its twin with a garbage burst in the middle, samples)."""
    from batch_common import six_variants
    ts, _ = tc.build_stream(600, events=False)
    bb = synth_dvbs.modulate(ts, 6, 5)
    rng = np.random.default_rng(1)
    x = bb * 75.0 + (rng.standard_normal(len(bb)) + 1j * rng.standard_normal(len(bb))) * 7.5
    iq = np.empty(2 * len(x), np.uint8)
    iq[0::2] = np.clip(np.rint(x.real + 128), 0, 255)
    iq[1::2] = np.clip(np.rint(x.imag + 128), 0, 255)
    n = len(x)
    twin = dict(six_variants(iq, n, BURST))["garbage burst in the middle"]
    return iq, twin, n


@pytest.mark.parametrize("engine", ["default", "viterbi", "hs"])
def test_end_to_end_on_the_decoders_ts(capi, ctx, engine):
    import bench_c1
    iq, twin, n = _captures()
    if engine == "hs":
        obj = capi.HsBatch(ctx, 2, n, 1.2)
    else:
        obj = capi.CaptureBatch(ctx, 2, n, 1.2, fec=capi.FEC12, anf=0, tile_len=4096, tile_warmup=512, viterbi=engine == "viterbi")
    bufs = [ctx.upload(iq), ctx.upload(twin)]
    try:
        res, ts = obj.decode([b.ptr for b in bufs], n)
        print(f"{engine}: clean {res[0]['ts_packets']} packets, with the burst {res[1]['ts_packets']}")
        # condition on the input
        assert res[0]["ts_packets"] >= 50 and res[1]["ts_packets"] < res[0]["ts_packets"], (res[0]["ts_packets"], res[1]["ts_packets"])
        got = obj.ts_census(res)
        for i in range(2):
            assert got[i] == tc.census(ts[i]) and got[i]["packets"] == res[i]["ts_packets"], (engine, i)
        # the clean capture behind acquisition: nothing lost — by the restatement over the slice and by the device from the same offset
        skip = bench_c1.SKIP_ACQ
        behind = tc.census(ts[0][188 * skip:])
        tb = capi.TsBatch(ctx, 1, res[0]["ts_packets"])
        try:
            dev, = tb.census([obj._fn("ts_dev")(obj.h, 0) + 188 * skip], [res[0]["ts_packets"] - skip])
        finally:
            tb.close()
        print(f"{engine}: behind {skip} packets: {behind['packets']} packets, cc_errors {behind['cc_errors']}; with the burst: cc_errors "
              f"{got[1]['cc_errors']}, cc_missing {got[1]['cc_missing']}")
        assert dev == behind and behind["cc_errors"] == 0 and behind["sync_errors"] == 0 and behind["tei"] == 0
        assert got[1]["cc_missing"] > 0
        fres, data, idx = obj.ts_filter(res, keep_pids=[tc.VIDEO])
        for i in range(2):
            assert data[i] == tc.select(ts[i], tc.kept(ts[i], [tc.VIDEO])) and fres[i]["kept"] * 188 == len(data[i]) > 0 and idx is None
    finally:
        obj.close()
        for b in bufs:
            b.free()
