"""lsdr_capture_each_run_async: every capture of a batch with its own length and its own tune (leandvb's --tune), both engines.

  1 ragged lengths: one batch of four lengths of the same capture, every TS against the reference BINARY's for that length;
  2 composition invariance, bit for bit: eight lengths (long, short, in front of the first detect point, around one block, around one
    chunk, none) in one batch against the same eight as the only capture of a one-capture object through the uniform entry point — result
    record, TS, symbols, detected bins, reports, Viterbi counts — for cu8 and cs16, and again with the lengths in reverse order;
  3 tuning: four carrier offsets, three of them outside the tiles' window, each tuned to its offset, against `leandvb --tune`; then
    lengths and tunes mixed;
  4 the reports of a tuned capture against the oracle's serial receiver constructed with set_freq;
  5 every refusal is LSDR_E_ARG with a message and leaves the object usable.

result.samples: rxb_geometry's rule — cstln_receiver runs over ((n − 1) // 128)·128 samples of the n it is given, and with anf = 1 auto_notch
hands it whole 4096-sample blocks only, so n is the capture's length rounded down to a block.
The reference binary (oracle/_ref/leandvb) is required: where it is missing these tests FAIL.
"""
import functools

import numpy as np
import pytest
from batch_common import REF_U8, capture, check_against_reference, references, shifted

pytestmark = pytest.mark.gpu

LSDR_E_ARG = -2
OMEGA = 1.2
FS = 2400e3
N_ALL = 1958423
# engine → (viterbi, noise_std, leandvb's extra arguments, pll_adjustment factor, tolerance dict)
ENGINES = {"default": (False, 7.5, (), 1.0, "TOL"), "viterbi": (True, 18.0, ("--viterbi",), 1.0 / 6.0, "LOW_SNR")}
LENGTHS = [1958423, 1500001, 1000000, 700001]
REF_PACKETS = {"default": [946, 712, 457, 302], "viterbi": [932, 698, 443, 288]}      # what the reference returns for LENGTHS
FREQS = [0.0, 1e-3, -1e-3, 3e-3]
REF_PACKETS_TUNED = {"default": 946, "viterbi": 932}                                  # … for every one of FREQS, tuned, whole capture
DEC = 64 * 4096                       # auto_notch::decimation lowered: 7 detect points in the whole capture, the first behind block 63
LENGTHS8 = [1958423, 700001, 200000, 4097, 4095, 129, 100, 0]


def _iq(engine):
    """The engine's capture and, for the Viterbi engine, the packets that were transmitted (the default graph's first packets include some
    that never were — the reference's own acquisition — so there the question is not asked: tests/test_gpu_capture_any.py)."""
    iq, sent = capture(1000, 11, ENGINES[engine][1])
    assert len(iq) == 2 * N_ALL
    return iq, sent if ENGINES[engine][0] else None


def _consumed(n, anf):
    n = n // 4096 * 4096 if anf else n
    return (n - 1) // 128 * 128 if n >= 129 else 0


def _make(capi, ctx, engine, n_captures, tile, anf, **kw):
    return capi.CaptureBatch(ctx, n_captures, N_ALL, OMEGA, anf=anf, tile_len=tile, tile_warmup=512, viterbi=ENGINES[engine][0], **kw)


def _symbols(cb, i, r):
    return (cb.soft(i, r["symbols"]) if cb.viterbi else cb.words(i, r["symbols"])).tobytes()


@functools.lru_cache(maxsize=None)
def _ragged(capi, ctx, engine, tile):
    """LENGTHS of the engine's capture in one each batch, anf = 1 (computed once): (results, TS)."""
    buf = ctx.upload(_iq(engine)[0])
    cb = _make(capi, ctx, engine, len(LENGTHS), tile, 1)
    try:
        return cb.decode_each([buf.ptr] * len(LENGTHS), LENGTHS)
    finally:
        cb.close()
        buf.free()


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [4096, 2048])
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_ragged_lengths_against_the_reference(capi, ctx, engine, tile):
    noise, extra = ENGINES[engine][1], ENGINES[engine][2]
    refs = references([(REF_U8 + extra, 1000, 11, noise, n) for n in LENGTHS])
    res, ts = _ragged(capi, ctx, engine, tile)
    sent = _iq(engine)[1]
    for i, n in enumerate(LENGTHS):
        check_against_reference(ts[i], refs[i], sent, REF_PACKETS[engine][i] - 10, f"{engine} tile {tile} length {n}", False)
        r = res[i]
        assert r["samples"] == _consumed(n, 1), (n, r)
        assert r["seam_bad"] == 0 and r["locked"] == 1, (n, r)
    assert len({r["tiles"] for r in res}) == len(LENGTHS)


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
def _everything(cb, i, r, ts):
    """All a capture produced, as comparable values."""
    rep = cb.reports(i)
    out = dict(res=r, ts=ts, sym=_symbols(cb, i, r), bins=cb.bins(i), rep={k: v.tobytes() for k, v in rep.items()}, n_rep=len(rep["freq"]))
    if cb.viterbi:
        st = cb.viterbi_stats(i)
        out["viterbi"] = (st["bytes"], st["symbols"])
    return out


@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_composition_invariance(capi, ctx, engine, fmt):
    iq = _iq(engine)[0]
    kw = {}
    if fmt == "cs16":                               # the same samples as 16-bit items, scaled back: s16 = 256·(u8 − 128), in_scale 2^-8
        iq = ((iq.astype(np.int16) - 128) * 256).astype(np.int16)
        kw = dict(in_format=capi.IN_CS16, in_scale=2.0 ** -8)
    kw.update(notch_decimation=DEC, reports=50000)
    buf = ctx.upload(iq)
    B = len(LENGTHS8)
    ptrs = [buf.ptr if n else None for n in LENGTHS8]
    try:
        # the yardstick: each length alone, through the uniform entry point
        alone = []
        for n in LENGTHS8:
            cb = _make(capi, ctx, engine, 1, 4096, 1, **kw)
            try:
                res, ts = cb.decode([buf.ptr], n)
                alone.append(_everything(cb, 0, res[0], ts[0]))
            finally:
                cb.close()
        # conditions on the input: the long captures decode, have detect points and reports; the short ones run through every early exit
        assert alone[0]["res"]["ts_packets"] > 900 and alone[1]["res"]["ts_packets"] > 250, (alone[0]["res"], alone[1]["res"])
        assert [len(a["bins"]) for a in alone] == [7, 2, 0, 0, 0, 0, 0, 0]
        assert [a["res"]["samples"] for a in alone] == [_consumed(n, 1) for n in LENGTHS8]
        assert [a["res"]["tiles"] > 0 for a in alone] == [True, True, True, True, False, False, False, False]
        assert alone[0]["n_rep"] == _consumed(LENGTHS8[0], 1) // 50000 and alone[3]["n_rep"] == 0
        cb = _make(capi, ctx, engine, B, 4096, 1, **kw)
        try:
            for order in (list(range(B)), list(reversed(range(B)))):
                res, ts = cb.decode_each([ptrs[k] for k in order], [LENGTHS8[k] for k in order])
                for i, k in enumerate(order):
                    got = _everything(cb, i, res[i], ts[i])
                    for what in got:
                        assert got[what] == alone[k][what], f"{engine} {fmt} length {LENGTHS8[k]} at place {i}: {what} is not the capture's own"
        finally:
            cb.close()
    finally:
        buf.free()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_tuning_against_the_reference(capi, ctx, engine):
    noise, extra = ENGINES[engine][1], ENGINES[engine][2]
    iq, sent = _iq(engine)

    def args(f):
        return REF_U8 + extra + ("--anf", "0", "--tune", repr(f * FS))

    refs = references([(args(f), 1000, 11, noise, None, f) for f in FREQS] + [(args(f), 1000, 11, noise, n, f) for f, n in zip(FREQS, LENGTHS)])
    # condition on the input: the reference decodes the tail of the unshifted capture whatever the offset, once tuned
    tail0 = refs[0][-188 * 800:]
    assert all(r[-188 * 800:] == tail0 for r in refs[:4])
    bufs = [ctx.upload(shifted(iq, f)) for f in FREQS]
    cb = _make(capi, ctx, engine, len(FREQS), 4096, 0)
    try:
        res, ts = cb.decode_each([b.ptr for b in bufs], [N_ALL] * len(FREQS), FREQS)
        for i, f in enumerate(FREQS):
            check_against_reference(ts[i], refs[i], sent, REF_PACKETS_TUNED[engine] - 10, f"{engine} offset {f} tuned", False)
            assert res[i]["seam_bad"] == 0 and res[i]["locked"] == 1 and res[i]["samples"] == _consumed(N_ALL, 0), res[i]
        # lengths and tunes mixed in one batch
        res, ts = cb.decode_each([b.ptr for b in bufs], LENGTHS, FREQS)
        for i, (f, n) in enumerate(zip(FREQS, LENGTHS)):
            check_against_reference(ts[i], refs[4 + i], sent, REF_PACKETS[engine][i] - 10, f"{engine} offset {f} tuned, length {n}", False)
            assert res[i]["seam_bad"] == 0 and res[i]["locked"] == 1 and res[i]["samples"] == _consumed(n, 0), res[i]
    finally:
        cb.close()
        for b in bufs:
            b.free()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
def report_deviations(capi, ctx, oracle, engine, f, period=65536, n=1 << 20):
    """The first n samples of the engine's capture shifted by f, twice in one batch tuned to f, against the oracle's serial receiver
    constructed with set_freq(f): per capture (max |ΔSS|/SS, max |ΔMER| in dB, max |ΔFREQ|) over all instants and `last`; each line is
    printed, and appended to the file LSDR_REPORTS_LOG names (how tolerance.py's entries are set)."""
    import os

    import pyoracle as po
    iq = (shifted(_iq(engine)[0], f) if f else _iq(engine)[0])[: 2 * n]
    o = oracle.rx(po.rx_params(sampler=1, cstln=1, omega=OMEGA, freq=f, meas_decimation=period, pll_adjustment=ENGINES[engine][3]), oracle.cconverter_u8(iq))
    st = o["state"]
    o_last = np.array([st.freqw / 65536.0, np.sqrt(np.float32(st.est_insp)), np.float32(10) * np.log10(np.float32(st.est_sp) / np.float32(st.est_ep))], np.float64)
    # condition on the input: the serial receiver, tuned, stays on the carrier
    assert len(o["freq"]) == o["consumed"] // period and abs(float(o["freq"].mean()) - f) <= 2e-4, o["freq"]
    buf = ctx.upload(iq)
    cb = _make(capi, ctx, engine, 2, 4096, 0, reports=period)
    out = []
    try:
        res, _ = cb.decode_each([buf.ptr, buf.ptr], [n, n], [f, f])
        for i in range(2):
            rep = cb.reports(i)
            assert res[i]["samples"] == o["consumed"] and len(rep["freq"]) == len(o["freq"])
            g = {k: np.append(rep[k], rep["last"][q]).astype(np.float64) for q, k in enumerate(("freq", "ss", "mer"))}
            w = {k: np.append(o[k], o_last[q]).astype(np.float64) for q, k in enumerate(("freq", "ss", "mer"))}
            assert all(np.isfinite(v).all() for v in g.values())
            d = (float(np.max(np.abs(g["ss"] - w["ss"]) / w["ss"])), float(np.max(np.abs(g["mer"] - w["mer"]))), float(np.max(np.abs(g["freq"] - w["freq"]))))
            line = (f"{engine} tune {f} capture {i}: instants {len(g['ss'])} max|dSS|/SS {d[0]:.5f} max|dMER| {d[1]:.4f} dB max|dFREQ| {d[2]:.3e} "
                    f"(oracle: FREQ mean {w['freq'].mean():.3e}; batch: FREQ mean {g['freq'].mean():.3e})")
            print(line)
            if os.environ.get("LSDR_REPORTS_LOG"):
                with open(os.environ["LSDR_REPORTS_LOG"], "a") as fh:
                    fh.write(line + "\n")
            out.append(d)
    finally:
        cb.close()
        buf.free()
    return out


@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_tuned_reports_against_the_oracle(capi, ctx, oracle, engine):
    from leansdr_amd import tolerance
    tol = getattr(tolerance, ENGINES[engine][4])
    freq_atol = tol.get("freq_atol_tuned", tol["freq_atol"])      # (a tuned bound exists only where the untuned one was measured to be exceeded)
    assert freq_atol < 0.5 * 1e-3, "a bound that a report of constant 0 would pass shows nothing"
    for d_ss, d_mer, d_freq in report_deviations(capi, ctx, oracle, engine, 1e-3):
        assert d_ss <= tol["ss_rtol"] and d_mer <= tol["mer_atol_db"] and d_freq <= freq_atol, (d_ss, d_mer, d_freq)


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_arguments(capi, ctx, engine):
    want_res, want_ts = _ragged(capi, ctx, engine, 4096)
    buf = ctx.upload(_iq(engine)[0])
    B = len(LENGTHS)
    cb = _make(capi, ctx, engine, B, 4096, 1)
    run = capi.lib.lsdr_capture_each_run_async
    ptrs = cb._ptrs([buf.ptr] * B)

    def refused(each, what, ptrs=ptrs):
        rc = run(cb.h, ptrs, each)
        msg = capi.lib.lsdr_last_error().decode()
        assert rc == LSDR_E_ARG and msg, (what, rc, msg)
        return msg

    try:
        e = cb.each(LENGTHS)
        e[2].n_samples = N_ALL + 1
        assert "samples" in refused(e, "n_samples > max_samples")
        for bad in (float("nan"), float("inf"), 0.5, -0.5, 0.75):
            e = cb.each(LENGTHS)
            e[1].tune = bad
            assert "tune" in refused(e, f"tune {bad}")
        e = cb.each(LENGTHS)
        e[3].reserved[4] = 1
        assert "reserved" in refused(e, "nonzero reserved")
        assert "pointer" in refused(cb.each(LENGTHS), "samples without a pointer", cb._ptrs([None] + [buf.ptr] * (B - 1)))
        cb.run_each_async([buf.ptr] * B, LENGTHS)
        assert "in flight" in refused(cb.each(LENGTHS), "a batch in flight")
        cb.wait()
        # the object is usable: the same batch again gives the first test's bytes
        res, ts = cb.decode_each([buf.ptr] * B, LENGTHS)
        assert res == want_res and ts == want_ts
    finally:
        cb.close()
        buf.free()
