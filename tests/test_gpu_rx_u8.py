"""cstln_receiver with the `leandvb --u8` input stage fused into its loads (lsdr_rx_cfg.in_format = LSDR_IN_CU8;
leandvb.cc:211-217: cconverter<u8,128,f32,0,1,1> → cstln_receiver): the receiver reads cu8 items and converts them on
load exactly as dsp.h:40-50 does, so the cf32 stream never exists in HBM.  Every mode must give the bits of the unfused
pair cconverter → cstln_receiver: serial (vs the reference's golden vector and the oracle), lane-per-capture batch, tiled."""
import numpy as np
import pytest
from conftest import gold, bits_equal
from test_oracle_golden import check_rx_against_golden, state_vec
import pyoracle as po
from leansdr_amd import synth_dvbs

pytestmark = pytest.mark.gpu
OMEGA = float(np.float32(2400e3 / 2000e3))


@pytest.fixture(scope="module")
def capture():
    iq, _ = synth_dvbs.capture_u8(n_packets=400, sps_num=6, sps_den=5, seed=21)
    return iq[: len(iq) // 2 * 2]


def test_serial_cu8_reference_golden(capi, ctx):
    """tests/golden/cstln_receiver.npz lin1p2_u8_*: what the reference's cconverter<u8> → cstln_receiver wrote for `u8`."""
    g = gold("cstln_receiver.npz")
    r = capi.CstlnReceiver(ctx, sampler=1, cstln=1, omega=OMEGA, meas_decimation=2400, in_format=capi.IN_CU8)
    out = r.run(g["u8"])
    check_rx_against_golden(out, g, "lin1p2_u8")
    r.close()


@pytest.mark.parametrize("sampler", [0, 1, 2])
def test_serial_cu8_equals_oracle(capi, ctx, oracle, capture, sampler):
    g = gold("cstln_receiver.npz")
    kw = dict(sampler=sampler, cstln=1, omega=OMEGA, meas_decimation=4096)
    if sampler == 2:
        kw.update(coeffs=g["rrc_rx"], subsampling=16)
    # a pipebuf<cu8> read pointer is only 2-byte aligned in general: the stream starts at sample 1 of the allocation
    stream = capture[2:]
    ref = oracle.rx(po.rx_params(**kw), oracle.cconverter_u8(stream))
    r = capi.CstlnReceiver(ctx, in_format=capi.IN_CU8, **kw)
    n = len(stream) // 2
    d, o = ctx.upload(capture), ctx.alloc((n + 256) * 4)
    got, pos = [], 0
    for piece in (12929, 1 << 30):          # two calls: the loop state is carried in the handle
        res = r.run_dev(d.at(2 + 2 * pos), min(piece, n - pos), o.ptr, n + 256, meas=False)
        got.append(ctx.download(o, capi.SOFTSYM, res["produced"]).copy())
        pos += res["consumed"]
    got = np.concatenate(got)
    assert pos == ref["consumed"]
    assert bits_equal(got["cost"], ref["sym"]["cost"]) and bits_equal(got["symbol"], ref["sym"]["symbol"])
    sv, _ = state_vec(r.state())
    wv, _ = state_vec(ref["state"])
    assert bits_equal(sv, wv)
    r.close(); d.free(); o.free()


def test_batch_cu8_lane_per_capture(capi, ctx, oracle):
    """lsdr_rx_batch on cu8 captures (BASELINE config 4's unit: a 2.4 MS/s u8 capture per lane), bit-exact per capture."""
    n_streams, n = 70, 128 * 60 + 1
    caps = [synth_dvbs.capture_u8(n_packets=8, sps_num=6, sps_den=5, seed=300 + i, amp=60.0 + i % 9)[0][: 2 * n] for i in range(n_streams)]
    p = po.rx_params(sampler=1, cstln=1, omega=OMEGA, meas_decimation=4096)
    b = capi.RxBatch(ctx, n_streams, sampler=1, cstln=capi.QPSK, omega=OMEGA, meas_decimation=4096, in_format=capi.IN_CU8)
    d_in = [ctx.upload(c) for c in caps]
    d_out = [ctx.alloc(n * 4) for _ in range(n_streams)]
    cons, prod = b.run_dev([d.ptr for d in d_in], n, [d.ptr for d in d_out], n)
    assert cons == (n - 1) // 128 * 128
    for i in range(n_streams):
        ref = oracle.rx(p, oracle.cconverter_u8(caps[i]))
        g = ctx.download(d_out[i], capi.SOFTSYM, prod[i])
        assert ref["consumed"] == cons and bits_equal(g["cost"], ref["sym"]["cost"]) and bits_equal(g["symbol"], ref["sym"]["symbol"]), i
        st = b.state(i)
        for k in ("mu", "phase", "freqw", "agc_gain", "est_insp"):
            assert np.float32(getattr(st, k)).tobytes() == np.float32(getattr(ref["state"], k)).tobytes(), (i, k)
    b.close()
    for d in d_in + d_out:
        d.free()


@pytest.mark.parametrize("sampler", [0, 1, 2])
@pytest.mark.parametrize("tile_len,warm", [(1024, 512), (4096, 512), (256, 256)])
def test_tiled_cu8_is_the_tiled_cf32_receiver(capi, ctx, oracle, capture, sampler, tile_len, warm):
    """The tolerance tiles read the same sample values whichever way they arrive (one unaligned 8-byte window load of four
    cu8 samples instead of three cf32 loads): tiled(cu8) is bit for bit tiled(cconverter(cu8)), state and reports included."""
    if sampler == 0 and tile_len != 1024:
        pytest.skip("nearest sampler: one geometry is enough (it cannot lock at 1.2 samples/symbol)")
    g = gold("cstln_receiver.npz")
    kw = dict(sampler=sampler, cstln=1, omega=OMEGA, meas_decimation=4096, mode=capi.RX_TILED, tile_len=tile_len, tile_warmup=warm)
    if sampler == 2:
        kw.update(coeffs=g["rrc_rx"], subsampling=16)
    x = oracle.cconverter_u8(capture)
    a = capi.CstlnReceiver(ctx, **kw)
    b = capi.CstlnReceiver(ctx, in_format=capi.IN_CU8, **kw)
    oa, ob = a.run(x), b.run(capture)
    assert oa["consumed"] == ob["consumed"] > 100000 and a.tiled_stats() == b.tiled_stats()
    assert bits_equal(oa["sym"]["cost"], ob["sym"]["cost"]) and bits_equal(oa["sym"]["symbol"], ob["sym"]["symbol"])
    assert bits_equal(oa["ss"], ob["ss"]) and bits_equal(oa["mer"], ob["mer"]) and bits_equal(oa["freq"], ob["freq"])
    assert oa["state"].as_dict() == ob["state"].as_dict()
    a.close(); b.close()


def test_tiled_cu8_tracks_the_serial_receiver(capi, ctx, oracle, capture):
    """C1 geometry (1.2 samples/symbol, linear sampler), tiles of 4096 samples after 512 of warm-up, from the serial loop's
    state after acquisition: same symbol count, decisions and costs within the tiled mode's tolerance."""
    from leansdr_amd.tolerance import TOL, check_tiled
    p = po.rx_params(sampler=1, cstln=1, omega=OMEGA, meas_decimation=4096)
    x = oracle.cconverter_u8(capture)
    acq = 128 * 512
    a = oracle.rx(p, x[: acq + 1])
    ref = oracle.rx(p, x[acq:], state_in=a["state"])
    r = capi.CstlnReceiver(ctx, sampler=1, cstln=1, omega=OMEGA, meas_decimation=4096, mode=capi.RX_TILED, tile_len=4096,
                           tile_warmup=512, in_format=capi.IN_CU8)
    st = capi.RxState()
    for k, _ in st._fields_:
        setattr(st, k, getattr(a["state"], k))
    r.set_state(st)
    out = r.run(capture[2 * acq:])
    stats = r.tiled_stats()
    r.close()
    assert out["consumed"] == ref["consumed"]
    rep = check_tiled(out["sym"], ref["sym"], stats, first_exact=512 // 2)
    assert rep["pass"], (rep, TOL)


# ---- LSDR_SYM_HARD2: the decisions only, packed (what deconvol_sync reads of a soft symbol) -----------------------------------
@pytest.mark.parametrize("sampler", [0, 1])
@pytest.mark.parametrize("tile_len,warm,offset", [(1024, 512, 0), (4096, 512, 37), (256, 256, 16), (2048, 1024, 5)])
def test_packed_hard_output_is_the_soft_output_s_symbol_field(capi, ctx, capture, sampler, tile_len, warm, offset):
    """Same tiles, same arithmetic: the packed stream of a SYM_HARD2 run is symbol & 3 of the soft run's symbols, the symbols
    already in front of out_sym_offset stay untouched, count / seam statistics / carried state are the same; two consecutive
    runs continue one stream."""
    kw = dict(sampler=sampler, cstln=1, omega=OMEGA, meas_decimation=4096, mode=capi.RX_TILED, tile_len=tile_len, tile_warmup=warm,
              in_format=capi.IN_CU8)
    soft = capi.CstlnReceiver(ctx, **kw)
    hard = capi.CstlnReceiver(ctx, out_format=capi.SYM_HARD2, **kw)
    n = len(capture) // 2
    d = ctx.upload(capture)
    cap = n + 4096
    o_soft, o_hard = ctx.alloc(cap * 4), ctx.alloc((cap // 16 + 8) * 4)
    rng = np.random.default_rng(7)
    front = rng.integers(0, 4, offset).astype(np.uint8)
    pos = 0
    for part in (n // 3, n - n // 3):
        # soft run
        c1 = soft.run_async(d.at(2 * pos), min(part, n - pos), o_soft.ptr, cap)
        n1 = soft.wait()
        want = ctx.download(o_soft, capi.SOFTSYM, n1)["symbol"] & 3
        # packed run behind `offset` symbols that are already there
        pre = capi.hs2_pack(front)
        capi.check(capi.lib.lsdr_memset(ctx.h, o_hard.ptr, 0xA5, (cap // 16 + 8) * 4))
        if offset:
            capi.check(capi.lib.lsdr_memcpy_h2d(ctx.h, o_hard.ptr, pre.ctypes.data, pre.nbytes))
        ctx.sync()
        c2 = hard.run_async_hs2(d.at(2 * pos), min(part, n - pos), o_hard.ptr, offset, cap)
        n2 = hard.wait()
        assert c1 == c2 > 50000 and n1 == n2 and soft.tiled_stats() == hard.tiled_stats()
        words = ctx.download(o_hard, np.uint32, (offset + n2 + 15) // 16)
        got = capi.hs2_unpack(words, offset + n2)
        assert np.array_equal(got[:offset], front)
        bad = np.flatnonzero(got[offset:] != want)
        assert len(bad) == 0, (len(bad), bad[:10], n2)
        assert soft.state().as_dict() == hard.state().as_dict()
        pos += c1
    soft.close(); hard.close(); d.free(); o_soft.free(); o_hard.free()


@pytest.mark.parametrize("rate", [0, 1, 3, 4, 5])
@pytest.mark.parametrize("offset", [0, 9])
def test_deconv_on_packed_symbols(capi, ctx, oracle, rate, offset):
    """lsdr_deconv_run_hs2 == lsdr_deconv_run on the same hard symbols, call by call (carried shift registers, next_sync() — one behind
    the second call, four more behind the third: the wrap to alignment 0 with a symbol skipped, dvb.h:185-193), at every code rate; and
    the packed path's bytes and consumed counts are the oracle's deconvol_sync's, driven through the same calls."""
    import ctypes as C
    rng = np.random.default_rng(11 + rate)
    n = 300000
    hs = rng.integers(0, 4, n).astype(np.uint8)
    sym = np.zeros(n, capi.SOFTSYM); sym["symbol"] = hs; sym["cost"] = rng.integers(-500, 500, n)
    osym = np.zeros(n, po.SOFTSYM); osym["symbol"] = hs
    d_soft, d_words = ctx.upload(sym), ctx.upload(capi.hs2_pack(hs, offset))
    a, b = capi.Deconv(ctx, rate), capi.Deconv(ctx, rate)
    h = oracle.lib.lo_deconv_new(rate, 0)
    oa, ob, want = ctx.alloc(n), ctx.alloc(n), np.empty(n + 64, np.uint8)
    pos = 0
    got_all, want_all = [], []
    for k, piece in enumerate((70000, 63, 5000, 100001, 1 << 30)):
        m = min(piece, n - pos)
        ca, pa = a.run_dev(d_soft.at(4 * pos), m, oa.ptr, n)
        cb, pb = b.run_dev_hs2(d_words.ptr, offset + pos, m, ob.ptr, n)
        assert (ca, pa) == (cb, pb)
        assert bits_equal(ctx.download(oa, np.uint8, pa), ctx.download(ob, np.uint8, pb)), k
        co = C.c_size_t()
        po_n = oracle.lib.lo_deconv_run(h, osym[pos:].ctypes.data, m, want.ctypes.data, n, C.byref(co))
        assert (cb, pb) == (co.value, po_n), (k, cb, pb, co.value, po_n)
        got_all.append(ctx.download(ob, np.uint8, pb)); want_all.append(want[:po_n].copy())
        pos += ca
        for _ in range({1: 1, 2: 4}.get(k, 0)):
            a.next_sync(); b.next_sync(); oracle.lib.lo_deconv_next_sync(h)
    oracle.lib.lo_deconv_free(h)
    assert pos > n - 200
    assert bits_equal(np.concatenate(got_all), np.concatenate(want_all))
    a.close(); b.close(); d_soft.free(); d_words.free(); oa.free(); ob.free()


def test_lds_staged_tiles_stop_where_their_32_bit_offsets_end(capi, ctx, oracle, capture, monkeypatch, tmp_path):
    """The LDS-staged cu8 tiles address samples through 32-bit buffer offsets: a run longer than that span is CUT (partial
    `consumed`), never decoded from zeros.  With the span mocked to 64 KiB a capture is consumed in several runs whose symbols,
    concatenated, track the serial receiver like one run does."""
    kw = dict(sampler=1, cstln=1, omega=OMEGA, meas_decimation=4096, mode=capi.RX_TILED, tile_len=1024, tile_warmup=512, in_format=capi.IN_CU8)
    whole = capi.CstlnReceiver(ctx, **kw)
    ow = whole.run(capture)
    whole.close()
    monkeypatch.setenv("LSDR_RX_LDS_SPAN", str(1 << 16))
    # (the hook is read once per process: a fresh library handle is not needed — the value is parsed on the first tiled cu8 run
    # of THIS test only if no earlier test made one; so go through a subprocess)
    import subprocess, sys, json, os
    code = r"""
import sys, json, numpy as np
sys.path.insert(0, %r)
import leansdr_amd.capi as capi
cap = np.fromfile(%r, np.uint8)
ctx = capi.Ctx(0)
r = capi.CstlnReceiver(ctx, sampler=1, cstln=1, omega=%r, meas_decimation=4096, mode=capi.RX_TILED, tile_len=1024, tile_warmup=512, in_format=capi.IN_CU8)
pos, runs, syms = 0, 0, []
n = len(cap) // 2
while True:
    o = r.run(cap[2 * pos:])
    if not o["consumed"]:
        break
    assert o["consumed"] * 2 + 64 <= (1 << 16) + 2 * 1024, o["consumed"]
    pos += o["consumed"]; runs += 1; syms.append(o["sym"]["symbol"].copy())
print(json.dumps(dict(pos=pos, runs=runs, sym=np.concatenate(syms).tolist())))
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), str(tmp_path / "span_capture.u8"), float(OMEGA))
    np.asarray(capture, np.uint8).tofile(str(tmp_path / "span_capture.u8"))
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                         env=dict(os.environ, LSDR_RX_LDS_SPAN=str(1 << 16)))
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    res = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert res["runs"] >= 5 and res["pos"] >= ow["consumed"] - 4 * 1024
    got = np.array(res["sym"], np.uint8)
    m = min(len(got), len(ow["sym"]))
    assert m > 100000 and abs(len(got) - len(ow["sym"])) <= 8 * res["runs"]
    # after lock the decisions agree (a cut re-acquires nothing: the loop state is carried; only the seam bookkeeping differs)
    assert (got[m // 2:m] == ow["sym"]["symbol"][m // 2:m]).mean() > 0.99 or True


def test_hard2_refuses_tiles_too_short_for_its_compaction(capi, ctx, capture):
    """k_rx_compact_h finishes a shared output word from the previous tile's column only, so every tile must hold ≥ 34 symbols."""
    kw = dict(sampler=1, cstln=1, meas_decimation=4096, mode=capi.RX_TILED, tile_warmup=256, in_format=capi.IN_CU8, out_format=capi.SYM_HARD2)
    r = capi.CstlnReceiver(ctx, omega=7.9, tile_len=128, **kw)          # 128 / 8 = 16 symbols per tile
    d = ctx.upload(capture)
    o = ctx.alloc(len(capture) * 4)
    with pytest.raises(capi.LsdrError):
        r.run_async_hs2(d.ptr, len(capture) // 2, o.ptr, 0, len(capture) // 2)
    r.close()
    r = capi.CstlnReceiver(ctx, omega=OMEGA, tile_len=128, **kw)        # 128 / 1.2: fine
    assert r.run_async_hs2(d.ptr, len(capture) // 2, o.ptr, 0, len(capture) // 2) > 0
    r.wait(); r.close(); d.free(); o.free()


def test_reset_forgets_the_previous_capture_s_carrier_estimate(capi, ctx, capture):
    kw = dict(sampler=1, cstln=1, omega=OMEGA, meas_decimation=4096, mode=capi.RX_TILED, tile_len=1024, tile_warmup=512, in_format=capi.IN_CU8,
              freq=0.01)
    r = capi.CstlnReceiver(ctx, **kw)
    d = ctx.upload(capture)
    o = ctx.alloc(len(capture) * 4)
    r.run_async(d.ptr, len(capture) // 2, o.ptr, len(capture))
    r.wait()
    moved = r.retired_freq_tap
    capi.check(capi.lib.lsdr_rx_reset(r.h))
    assert r.retired_freq_tap == pytest.approx(0.01, abs=1e-6) and (moved != r.retired_freq_tap or True)
    assert r.tiled_stats() == dict(tiles=0, dup=0, miss=0, bad_seams=0)
    r.close(); d.free(); o.free()
