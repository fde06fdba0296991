"""lsdr_capture_batch's signal reports (lsdr_capture_reports_set / lsdr_capture_reports_get): per capture what `leandvb --fd-info` prints —
cstln_receiver's FREQ, SS and MER once per meas_decimation samples (sdr.h:857-913) — from the batch's own launches, both engines.

  1 against the oracle's serial chain cconverter_u8 → [auto_notch] → rx(meas_decimation = period): the same number of reports, every one
    within leansdr_amd.tolerance's ss_rtol / mer_atol_db / freq_atol, and `last` within them of the oracle's end state;
  2 reports inside tile 0 have the oracle's float32 bits;
  3 a carrier offset shows in FREQ (a report of constant 0 fails);
  4 reports change nothing else: results, TS and symbols of an object with reports are those of one without;
  5 a capture's reports do not depend on its neighbours in the batch, nor on aux_cus;
  6 the cs16 form of the same signal;
  7 errors.

LSDR_REPORTS_LOG=<file>: every compared instant's deviations, one line per capture (how the freq_atol entries were set:
profiles/capture_batch_reports/deviation.txt).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
from batch_common import capture

pytestmark = pytest.mark.gpu

LSDR_E_ARG = -2
N = 1 << 20
DEC = 64 * 4096                     # auto_notch::decimation lowered: 3 detect points in 1 Mi samples
OMEGA = 1.2
# engine → (viterbi, noise_std, pll_adjustment factor, tolerance dict name, carrier offset of test 3 in cycles per sample)
ENGINES = {"default": (False, 7.5, 1.0, "TOL", 1e-4), "viterbi": (True, 18.0, 1.0 / 6.0, "LOW_SNR", 2e-4)}


def _tol(engine):
    from leansdr_amd import tolerance
    return getattr(tolerance, ENGINES[engine][3])


@functools.lru_cache(maxsize=None)
def _captures(engine, anf, offset=0.0):
    """Two cu8 captures of N samples at the engine's noise; anf: with test_soft_symbols_against_the_oracle_chain's CW; offset: rotated by
    that many cycles per sample before re-quantising."""
    out = []
    for k in range(2):
        iq = capture(600, 41 + k, ENGINES[engine][1])[0][: 2 * N]
        if anf or offset:
            t = np.arange(N)
            x = (iq[0::2].astype(np.float64) - 128) + 1j * (iq[1::2].astype(np.float64) - 128)
            if offset:
                x = x * np.exp(2j * np.pi * offset * t)
            if anf:
                f = np.where(t < 2 * DEC + 4096 * 5, 0.1234, -0.31)
                x = x + 14.0 * np.exp(1j * 2 * np.pi * np.cumsum(f))
            iq = np.empty(2 * N, np.uint8)
            iq[0::2] = np.clip(np.rint(x.real + 128), 0, 255)
            iq[1::2] = np.clip(np.rint(x.imag + 128), 0, 255)
        out.append(np.ascontiguousarray(iq))
    return out


_ORACLE = {}


def _oracle_chain(oracle, engine, anf, period, k, offset=0.0, n=N):
    """The serial chain's reports for capture k: dict(freq, ss, mer, last = [freq, ss, mer] of the end state, consumed)."""
    import pyoracle as po
    key = (engine, anf, period, k, offset, n)
    if key not in _ORACLE:
        xf = oracle.cconverter_u8(_captures(engine, anf, offset)[k][: 2 * n])
        if anf:
            xf, _ = oracle.auto_notch(xf, 1, DEC)
        o = oracle.rx(po.rx_params(sampler=1, cstln=1, omega=OMEGA, meas_decimation=period, pll_adjustment=ENGINES[engine][2]), xf)
        st = o["state"]
        mer = np.float32(10) * np.log10(np.float32(st.est_sp) / np.float32(st.est_ep)) if st.est_ep else np.float32(0)
        _ORACLE[key] = dict(freq=o["freq"].copy(), ss=o["ss"].copy(), mer=o["mer"].copy(), consumed=int(o["consumed"]),
                            last=np.array([st.freqw / 65536.0, np.sqrt(np.float32(st.est_insp)), mer], np.float32))
        assert len(o["freq"]) == o["consumed"] // period
    return _ORACLE[key]


def _run(capi, ctx, arrays, n, engine, anf, tile, period, aux_cus=0, symbols=False, **kw):
    """One batch of the first n samples of `arrays` (two values per sample): results, TS, reports per capture (None with period 0)."""
    bufs = [ctx.upload(a[: 2 * n]) for a in arrays]
    cb = capi.CaptureBatch(ctx, len(arrays), n, OMEGA, anf=anf, tile_len=tile, tile_warmup=512, notch_decimation=DEC if anf else 0,
                           viterbi=ENGINES[engine][0], aux_cus=aux_cus, reports=period, **kw)
    try:
        res, ts = cb.decode([b.ptr for b in bufs], n)
        out = dict(res=res, ts=ts, rep=[cb.reports(i) if period else None for i in range(len(arrays))], sym=[])
        if symbols:
            for i, r in enumerate(res):
                out["sym"].append((cb.soft(i, r["symbols"]) if cb.viterbi else cb.words(i, r["symbols"])).tobytes())
    finally:
        cb.close()
        for b in bufs:
            b.free()
    return out


def _deviations(rep, o, name, first=0):
    """max |ΔSS|/SS, |ΔMER| in dB, |ΔFREQ| over the instants from `first` on and of `last`; logged where LSDR_REPORTS_LOG is set."""
    assert len(rep["freq"]) == len(rep["ss"]) == len(rep["mer"]) == len(o["freq"]), f"{name}: {len(rep['freq'])} reports, the oracle {len(o['freq'])}"
    g = {k: np.append(rep[k][first:], rep["last"][i]).astype(np.float64) for i, k in enumerate(("freq", "ss", "mer"))}
    w = {k: np.append(o[k][first:], o["last"][i]).astype(np.float64) for i, k in enumerate(("freq", "ss", "mer"))}
    assert all(np.isfinite(v).all() for v in g.values()), name
    d = dict(ss=float(np.max(np.abs(g["ss"] - w["ss"]) / w["ss"])), mer=float(np.max(np.abs(g["mer"] - w["mer"]))),
             freq=float(np.max(np.abs(g["freq"] - w["freq"]))))
    line = (f"{name}: instants {len(g['ss'])} max|dSS|/SS {d['ss']:.5f} max|dMER| {d['mer']:.4f} dB max|dFREQ| {d['freq']:.3e} "
            f"(oracle: SS {w['ss'].mean():.2f} MER {w['mer'].mean():.2f} dB FREQ mean {w['freq'].mean():.3e})")
    print(line)
    log = os.environ.get("LSDR_REPORTS_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    return d


def _within(d, tol, name):
    assert d["ss"] <= tol["ss_rtol"], f"{name}: SS {d['ss']:.5f} off, bound {tol['ss_rtol']}"
    assert d["mer"] <= tol["mer_atol_db"], f"{name}: MER {d['mer']:.4f} dB off, bound {tol['mer_atol_db']}"
    assert d["freq"] <= tol["freq_atol"], f"{name}: FREQ {d['freq']:.3e} off, bound {tol['freq_atol']}"


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [65536, 50000])
@pytest.mark.parametrize("anf,tile", [(0, 4096), (1, 4096), (1, 2048)])
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_against_the_oracle_chain(capi, ctx, oracle, engine, anf, tile, period):
    caps = _captures(engine, anf)
    got = _run(capi, ctx, caps, N, engine, anf, tile, period)
    for k in range(2):
        o = _oracle_chain(oracle, engine, anf, period, k)
        name = f"{engine} anf {anf} tile {tile} period {period} capture {k}"
        assert got["res"][k]["samples"] == o["consumed"], name
        assert len(got["rep"][k]["freq"]) == o["consumed"] // period, name
        _within(_deviations(got["rep"][k], o, name), _tol(engine), name)


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_tile_0_is_exact(capi, ctx, oracle, engine):
    """8192 samples, a report per chunk: the first four lie in tile 0 (512 samples), the reference's arithmetic."""
    n = 8192
    caps = [c[: 2 * n] for c in _captures(engine, 0)]
    got = _run(capi, ctx, caps, n, engine, 0, 4096, 128)
    for k in range(2):
        o = _oracle_chain(oracle, engine, 0, 128, k, n=n)
        rep = got["rep"][k]
        assert len(rep["freq"]) == 63 and len(o["freq"]) == 63
        for f in ("freq", "ss", "mer"):
            assert rep[f][:4].tobytes() == o[f][:4].tobytes(), f"{engine} capture {k}: {f} {rep[f][:4]} is not the oracle's {o[f][:4]}"
        assert np.isfinite(rep["last"]).all()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_carrier_offset_shows(capi, ctx, oracle, engine):
    offset, period = ENGINES[engine][4], 65536
    tol = _tol(engine)
    assert tol["freq_atol"] < 0.5 * offset, "a bound that a report of constant 0 would pass shows nothing"
    caps = _captures(engine, 0, offset)
    got = _run(capi, ctx, caps, N, engine, 0, 4096, period)
    first = 200000 // period                      # instant q is at sample (q + 1)·period
    assert (first + 1) * period > 200000 >= first * period
    for k in range(2):
        o = _oracle_chain(oracle, engine, 0, period, k, offset)
        # condition on the input: the serial receiver reports the offset
        assert abs(float(o["freq"].mean()) - offset) <= 0.2 * offset, f"invalid input: the oracle's mean FREQ is {o['freq'].mean():.3e} at an offset of {offset}"
        name = f"{engine} offset {offset} capture {k}"
        d = _deviations(got["rep"][k], o, name, first=first)
        assert d["freq"] <= tol["freq_atol"], f"{name}: FREQ {d['freq']:.3e} off, bound {tol['freq_atol']}"
        assert abs(float(got["rep"][k]["freq"][first:].mean()) - offset) <= 0.2 * offset + tol["freq_atol"], name


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine,anf", [("default", 1), ("viterbi", 1), ("default", 0), ("viterbi", 0)])
def test_reports_change_nothing_else(capi, ctx, engine, anf):
    caps = _captures(engine, anf)
    on = _run(capi, ctx, caps, N, engine, anf, 4096, 50000, symbols=True)
    off = _run(capi, ctx, caps, N, engine, anf, 4096, 0, symbols=True)
    for k in range(2):
        assert off["res"][k]["ts_packets"] > 400, off["res"][k]      # condition on the input: it decodes
        assert on["res"][k] == off["res"][k], (k, on["res"][k], off["res"][k])
        assert on["ts"][k] == off["ts"][k], f"capture {k}: TS differs"
        assert on["sym"][k] == off["sym"][k], f"capture {k}: symbols differ"
        assert len(on["rep"][k]["ss"]) == on["res"][k]["samples"] // 50000


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_neighbours_do_not_matter(capi, ctx, engine):
    caps = _captures(engine, 1)
    n = 1 << 19
    alone = _run(capi, ctx, [caps[0]], n, engine, 1, 4096, 50000)["rep"][0]
    three = _run(capi, ctx, [caps[1], caps[0], caps[1]], n, engine, 1, 4096, 50000)["rep"][1]
    aux = _run(capi, ctx, [caps[1], caps[0], caps[1]], n, engine, 1, 4096, 50000, aux_cus=8)["rep"][1]
    assert len(alone["ss"]) == ((n // 4096 * 4096 - 1) // 128 * 128) // 50000
    for f in ("freq", "ss", "mer", "last"):
        assert alone[f].tobytes() == three[f].tobytes(), f"{f}: batch of 1 {alone[f]}, batch of 3 {three[f]}"
        assert alone[f].tobytes() == aux[f].tobytes(), f"{f}: without aux_cus {alone[f]}, with {aux[f]}"


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_cs16_form_of_the_same_signal(capi, ctx, oracle, engine):
    """capture_s16: the same analogue signal quantised 256 times finer, scaled back by in_scale = 2^-8 — against the cu8 capture's oracle values."""
    from leansdr_amd import synth_dvbs
    period = 65536
    caps = [np.ascontiguousarray(synth_dvbs.capture_s16(600, sps_num=6, sps_den=5, seed=41 + k, noise_std=ENGINES[engine][1])[0][: 2 * N]) for k in range(2)]
    got = _run(capi, ctx, caps, N, engine, 0, 4096, period, in_format=capi.IN_CS16, in_scale=2.0 ** -8)
    tol = _tol(engine)
    for k in range(2):
        o = _oracle_chain(oracle, engine, 0, period, k)
        name = f"{engine} cs16 capture {k}"
        d = _deviations(got["rep"][k], o, name)
        assert d["ss"] <= tol["ss_rtol"] and d["mer"] <= tol["mer_atol_db"], (name, d)


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
def test_errors(capi, ctx):
    caps = [c[: 2 * 65536] for c in _captures("default", 0)]
    bufs = [ctx.upload(c) for c in caps]
    cb = capi.CaptureBatch(ctx, 2, 65536, OMEGA, anf=0)
    try:
        n, last = C.c_size_t(), capi.CaptureReport()
        buf = (capi.CaptureReport * 8)()
        get = capi.lib.lsdr_capture_reports_get
        assert capi.lib.lsdr_capture_reports_set(cb.h, 64) == LSDR_E_ARG
        assert capi.lib.lsdr_capture_reports_set(cb.h, 127) == LSDR_E_ARG
        assert get(cb.h, 0, buf, 8, C.byref(n), C.byref(last)) == LSDR_E_ARG          # reports are off
        with pytest.raises(capi.LsdrError):
            capi.CaptureBatch(ctx, 2, 65536, OMEGA, anf=0, reports=64)
        cb.set_reports(4096)
        cb.run_async([b.ptr for b in bufs], 65536)
        assert capi.lib.lsdr_capture_reports_set(cb.h, 8192) == LSDR_E_ARG            # a batch is in flight
        assert get(cb.h, 0, buf, 8, C.byref(n), C.byref(last)) == LSDR_E_ARG
        res = cb.wait()
        assert get(cb.h, 2, buf, 8, C.byref(n), C.byref(last)) == LSDR_E_ARG          # no such capture
        assert get(cb.h, -1, buf, 8, C.byref(n), C.byref(last)) == LSDR_E_ARG
        full = cb.reports(1)
        want = res[1]["samples"] // 4096
        assert want == 15 and len(full["ss"]) == want
        for i in range(8):
            buf[i].ss = -1.0
        assert get(cb.h, 1, buf, 3, C.byref(n), None) == 0 and n.value == want         # cap < *n: cap entries, the full count
        assert [buf[i].ss for i in range(3)] == [float(v) for v in full["ss"][:3]] and buf[3].ss == -1.0
        assert get(cb.h, 1, None, 0, C.byref(n), C.byref(last)) == 0 and n.value == want and last.ss == float(full["last"][1])
        cb.set_reports(0)                                                               # off again
        assert get(cb.h, 0, buf, 8, C.byref(n), C.byref(last)) == LSDR_E_ARG
        cb.run_async([b.ptr for b in bufs], 65536)
        assert cb.wait()[1] == res[1]
    finally:
        cb.close()
        for b in bufs:
            b.free()
