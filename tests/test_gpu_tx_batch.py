"""lsdr_tx_batch on the GPU: every stream of a batch is bit for bit oracle.chansim(oracle.tx_chain(ts_i, …), …) — what leandvbtx |
leanchansim write for that stream alone — in both output formats, alone, at any position of a batch and on a reused object; the noise
stage's further rounds leave the same bytes; the launches do not depend on the number of streams; and the captures decode where they lie.

The ragged batch: six streams of 0, 5, 12, 13, 40 and 100 packets at 6/5 with AGC, one code rate each.  100 packets are the smallest
size that crosses what can go wrong: 1361 AGC chunks (more than one 64-chunk step of the EMA walk), 86 sample tiles, and a noise stage
of more than 50 count/scan blocks of 4096 candidate pairs.
"""
import hashlib

import numpy as np
import pytest

from conftest import bits_equal, gold
from leansdr_amd import synth_dvbs

pytestmark = pytest.mark.gpu

NPK = [0, 5, 12, 13, 40, 100]
#            fec  amp / power_db            scale  noise                   seed
EACH = [dict(fec=0, amp=75.0, scale=1.0, awgn_db=10.0, seed=1),
        dict(fec=1, amp=30.0, scale=0.5, awgn_db=3.0, seed=2),
        dict(fec=3, power_db=37.5, scale=2.0, awgn_db=0.0, seed=None),           # --deterministic: the unseeded generator
        dict(fec=4, amp=10.0, scale=0.0, noise_stddev=0.0, seed=4),              # scale 0 means 1; no noise, the adder still runs
        dict(fec=5, amp=75.0, scale=0.8, awgn_db=17.5, seed=5),
        dict(fec=0, amp=60.0, scale=1.1, awgn_db=12.0, seed=123456789)]


def _amp(capi, e):
    return e["amp"] if "amp" in e else capi.db_to_amplitude(e["power_db"])


def oracle_capture(capi, oracle, ts, e, ou8, interp=6, decim=5, agc=True, cstln=1):
    """(what leandvbtx | leanchansim write, the drand48 state behind the last noise sample)"""
    y = oracle.tx_chain(ts, interp=interp, decim=decim, amp=_amp(capi, e), agc=agc, cstln=cstln, rate=e["fec"])
    awgn = e.get("awgn_db") if "noise_stddev" not in e else None
    out = oracle.chansim(y, awgn_db=awgn, scale=e["scale"] or 1.0, ou8=ou8, seed=e["seed"])
    stddev = capi.db_to_amplitude(awgn) if awgn is not None else 0.0
    return out, oracle.wgn(len(y), stddev, e["seed"])[1]


@pytest.fixture(scope="module")
def streams():
    return [synth_dvbs.ts_packets(n, start=1000 * i) for i, n in enumerate(NPK)]


@pytest.fixture(scope="module")
def want(capi, oracle, streams):
    """The oracle's captures of the ragged batch, once: {ou8: [(samples, noise state)]}"""
    return {ou8: [oracle_capture(capi, oracle, ts, e, ou8) for ts, e in zip(streams, EACH)] for ou8 in (False, True)}


def make(capi, ctx, B, ou8=False, max_packets=100, **kw):
    kw = dict(dict(interp=6, decim=5, agc=True), **kw)
    return capi.TxBatch(ctx, B, max_packets, out_format=capi.IN_CU8 if ou8 else capi.IN_CF32, **kw)


@pytest.mark.parametrize("ou8", [False, True])
def test_ragged_batch_is_the_oracle(capi, ctx, streams, want, ou8):
    tb = make(capi, ctx, 6, ou8)
    try:
        res = tb.run(streams, EACH)
        got = tb.download_all()
        for i, (r, e) in enumerate(zip(res, EACH)):
            plan = tb.plan(e, n_packets=NPK[i])
            assert {k: r[k] for k in plan} == plan, i
            ref, state = want[ou8][i]
            assert r["samples"] == len(ref) and bits_equal(got[i], ref), i
            assert r["noise_state"] == state and r["noise_rounds"] == (1 if len(ref) else 0), (i, r)
        assert [r["samples"] > 0 for r in res] == [False, False, True, True, True, True]
        assert res[5]["samples"] // 128 == 1361 and res[5]["agc_estimated"] > 0
    finally:
        tb.close()


def test_position_independence_and_reuse(capi, ctx, streams, want):
    ref = [w[0] for w in want[False]]
    one = make(capi, ctx, 1)
    six = make(capi, ctx, 6)
    try:
        one.run([streams[5]], [EACH[5]])
        assert bits_equal(one.download(0), ref[5])
        perm = [3, 5, 0, 4, 1, 2]
        six.run([streams[k] for k in perm], [EACH[k] for k in perm])
        got = six.download_all()
        for slot, k in enumerate(perm):
            assert bits_equal(got[slot], ref[k]), (slot, k)
        # the same object again, other streams in every slot: what a fresh object gives (test_ragged_batch_is_the_oracle)
        six.run(streams, EACH)
        got = six.download_all()
        for k in range(6):
            assert bits_equal(got[k], ref[k]), k
        one.run([streams[4]], [EACH[4]])
        assert bits_equal(one.download(0), ref[4])
    finally:
        one.close(); six.close()


def test_against_the_one_stream_blocks(capi, ctx, oracle, streams, want):
    """TxChain → Wgn(add = scale·y) → cconverter, the whole stream in one call: the same bytes as stream 4 of the batch."""
    e = EACH[4]
    tx = capi.TxChain(ctx, interp=6, decim=5, amp=e["amp"], agc=True, rate=e["fec"])
    y = tx.run(streams[4])
    tx.close()
    w = capi.Wgn(ctx, e["seed"])
    z = w.run(len(y), capi.db_to_amplitude(e["awgn_db"]), add=oracle.scaler(e["scale"], y))
    state = w.state
    w.close()
    u8 = capi.cconv_f32_u8(ctx, z)
    tb = make(capi, ctx, 1, ou8=True, max_packets=40)
    try:
        res = tb.run([streams[4]], [e])
        assert bits_equal(tb.download(0), u8) and res[0]["noise_state"] == state
    finally:
        tb.close()
    assert np.array_equal(z, want[False][4][0])                           # (the drifter's identity rotation: signed zeros at most)


@pytest.mark.parametrize("cstln,fec,interp", [(2, 1, 3), (3, 3, 3), (0, 0, 2)])
def test_other_constellations(capi, ctx, oracle, cstln, fec, interp):
    """8PSK 2/3 and 16APSK 3/4 at interp 3, BPSK 1/2 at interp 2: 30 packets, no AGC, cf32."""
    ts = [synth_dvbs.ts_packets(30), synth_dvbs.ts_packets(30, start=77)]
    each = [dict(fec=fec, amp=75.0, scale=1.0, awgn_db=6.0, seed=11), dict(fec=fec, amp=20.0, scale=1.5, awgn_db=-3.0, seed=12)]
    tb = make(capi, ctx, 2, max_packets=30, interp=interp, decim=1, agc=False, cstln=cstln)
    try:
        tb.run(ts, each)
        got = tb.download_all()
        for i in range(2):
            ref, _ = oracle_capture(capi, oracle, ts[i], each[i], False, interp=interp, decim=1, agc=False, cstln=cstln)
            assert len(ref) > 0 and bits_equal(got[i], ref), i
    finally:
        tb.close()


def test_goldens(capi, ctx):
    """The stage in front of the channel against leandvbtx's own output (tests/golden/tx.npz): scale 1 and noise_stddev 0 still pass
    the adder and the identity rotation, which change a −0.0 only.  All six cf32 cases of test_oracle_tx.CASES are kept: the oracle's
    streams hold no −0.0 (f4_cr34 holds 395 values +0.0, psk8_23 two, which the channel leaves as they are)."""
    from test_oracle_tx import CASES
    g = gold("tx.npz")
    for name, kw in CASES:
        kw = dict(kw)
        tb = capi.TxBatch(ctx, 2, len(g["ts"]), interp=kw.pop("interp"), decim=kw.pop("decim", 1), cstln=kw.pop("cstln", capi.QPSK),
                          agc=kw.pop("agc", False))
        try:
            e = dict(fec=kw.pop("rate", 0), amp=kw.pop("amp", 1.0), scale=1.0, noise_stddev=0.0, seed=None)
            assert not kw
            res = tb.run([g["ts"], g["ts"]], [e, e])
            for y in tb.download_all():
                assert len(y) == int(g[name + "_n"]) == res[0]["samples"], name
                assert hashlib.sha256(y.tobytes()).digest() == bytes(g[name + "_sha"]), name
        finally:
            tb.close()


def test_short_fall_rounds(capi, ctx, streams, want):
    tb = make(capi, ctx, 1)
    try:
        tb.set_noise_margin(-6.0)                                         # round 1's candidates end about 6 σ before the last sample
        res = tb.run([streams[5]], [EACH[5]])
        assert res[0]["noise_rounds"] >= 2, res
        assert bits_equal(tb.download(0), want[False][5][0]) and res[0]["noise_state"] == want[False][5][1]
    finally:
        tb.close()


def test_launches_do_not_depend_on_the_streams(capi, ctx, streams):
    n = []
    for B in (1, 6):
        tb = make(capi, ctx, B, max_packets=40)
        try:
            tb.run([streams[4]] * B, [EACH[4]] * B)
            n.append(tb.stats())
        finally:
            tb.close()
    assert n[0]["launches_last_run"] == n[1]["launches_last_run"] > 0 and n[0]["runs"] == n[1]["runs"] == 1, n


def test_arguments(capi, ctx, streams):
    import ctypes as C
    for bad in (dict(interp=0), dict(decim=0), dict(out_format=2), dict(out_format=-1)):
        with pytest.raises(capi.LsdrError, match="lsdr error -2"):
            capi.TxBatch(ctx, 1, 40, **bad)
    cfg = capi.TxBatch(None, 1, 40).cfg
    cfg.reserved[3] = 1
    h = C.c_void_p()
    assert capi.lib.lsdr_tx_batch_create(ctx.h, C.byref(cfg), C.byref(h)) == -2
    tb = make(capi, ctx, 1, max_packets=40)
    try:
        e = tb.each(**EACH[4])
        e.reserved[2] = 1
        with pytest.raises(capi.LsdrError, match="lsdr error -2"):
            tb.run_async([streams[4]], [e])
        with pytest.raises(capi.LsdrError, match="lsdr error -2"):        # n_packets > max_packets
            tb.run_async([streams[5]], [EACH[5]])
        with pytest.raises(capi.LsdrError, match="lsdr error -2"):        # a rate QPSK cannot carry: lsdr_convol_create's code
            tb.run_async([streams[4]], [dict(EACH[4], fec=6)])
        tb.run_async([streams[4]], [EACH[4]])
        with pytest.raises(capi.LsdrError, match="lsdr error -2"):        # a second run before wait
            tb.run_async([streams[3]], [EACH[3]])
        res = tb.wait()
        assert res[0]["samples"] == tb.plan(EACH[4], n_packets=40)["samples"]
    finally:
        tb.close()


def test_loopback_without_pcie(capi, ctx):
    """B = 4 captures of 600 packets (6/5, rate 1/2, amp 75 with AGC as the reference's benchmark makes them, noise 7.5, cu8) decoded
    from the generator's device pointers: byte for byte the TS of an uploaded copy, only sent packets but the first 12, at least half."""
    B, npk = 4, 600
    ts = [synth_dvbs.ts_packets(npk, start=5000 * i) for i in range(B)]
    tb = make(capi, ctx, B, ou8=True, max_packets=npk)
    cb = None
    try:
        tb.run(ts, [dict(fec=0, amp=75.0, scale=1.0, noise_stddev=7.5, seed=100 + i) for i in range(B)])
        n = tb.lengths()
        cb = capi.CaptureBatch(ctx, B, max(n), 1.2, fec=capi.FEC12)
        res, got = cb.decode_each(tb.ptrs(), n)
        iq = tb.download_all()
        bufs = [ctx.upload(a) for a in iq]
        res2, got2 = cb.decode_each([d.ptr for d in bufs], n)
        for d in bufs:
            d.free()
        for i in range(B):
            x = iq[i].astype(np.float64) - 128
            rms = np.sqrt(np.mean(x[:, 0] ** 2 + x[:, 1] ** 2))
            assert 19 <= rms <= 75, (i, rms)
            assert got[i] == got2[i] and res[i]["ts_packets"] == res2[i]["ts_packets"], i
            pk = np.frombuffer(got[i], np.uint8).reshape(-1, 188)
            sent = {bytes(t) for t in ts[i]}
            good = sum(bytes(t) in sent for t in pk)
            print(f"loopback stream {i}: rms {rms:.1f}, {len(pk)} packets back, {good} of them sent")
            assert good >= len(pk) - 12 and len(pk) >= npk // 2, (i, len(pk), good)
    finally:
        tb.close()
        if cb:
            cb.close()
