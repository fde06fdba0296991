"""LSDR_RX_TILED beyond QPSK-by-arithmetic: BPSK (R = 2 rotations), 8PSK (R = 8), the table-gather slicer of the tile kernel
(every constellation but QPSK; QPSK under LSDR_RX_NO_ARITH or harden), harden, allow_drift with a tuned receiver, the BPSK branch
of the SS / MER estimators — against the oracle's exact serial receiver continued from the same acquisition state.

The streams (tests/rx_tiled_common.py) carry a small carrier offset, so that the phase a tile re-acquires from 0 falls on EVERY
rotation of the constellation in turn: each row of the relabel table, the moduli of the rotation bookkeeping (quad = 65536 / R,
rmask = R − 1) and rx_rotate_back are exercised for R = 2, 4 and 8.  tests/test_oracle_rx_tile_emulation.py asserts, with the
oracle alone, that this is so and that the tile algorithm holds on these streams; the bounds (leansdr_amd.tolerance: TOL_BPSK,
TOL_PSK8, and TOL itself for QPSK) come from that emulation, not from the GPU.
"""
import numpy as np
import pytest
from conftest import bits_equal
import pyoracle as po
import rx_tiled_common as tc
from leansdr_amd import tolerance
from leansdr_amd.tolerance import TOL, TOL_PSK8, check_tiled

pytestmark = pytest.mark.gpu

GEO_IDS = [f"{g[0]}-{g[1]}" for g in tc.GEOMETRIES]


@pytest.fixture(scope="module")
def refs(oracle):
    """Per case (and "drift": the QPSK stream DRIFT_FREQ off, receiver tuned there with allow_drift): the stream, the receiver's
    keywords, the serial oracle's state after acquisition and its continuation — computed once, never modified."""
    out = {}
    for name in [c["name"] for c in tc.CASES] + ["drift"]:
        drift = name == "drift"
        case = tc.CASE_BY_NAME["qpsk12_table" if drift else name]
        kw = tc.rx_kwargs(case, **(dict(freq=tc.DRIFT_FREQ, allow_drift=1) if drift else {}))
        x = tc.case_stream(oracle, case, shift=tc.DRIFT_FREQ if drift else 0.0)
        st, ref = tc.acquire(oracle, po.rx_params(**kw), x)
        out[name] = dict(case=case, kw=kw, x=x, tail=x[tc.ACQ:], st=st, ref=ref, tol=getattr(tolerance, case["tol"]))
    return out


def gpu_state(capi, st, **fields):
    g = capi.RxState()
    for k, _ in g._fields_:
        setattr(g, k, getattr(st, k))
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def tiled_receiver(capi, ctx, kw, st, geometry, **more):
    r = capi.CstlnReceiver(ctx, mode=capi.RX_TILED, tile_len=geometry[0], tile_warmup=geometry[1], **dict(kw, **more))
    r.set_state(st if isinstance(st, capi.RxState) else gpu_state(capi, st))
    return r


def assert_tiled_is_serial(out, stats, ref, tol, geometry, reports=True):
    """What tests/test_gpu_rx_tiled.py::test_tiled_vs_serial asserts, under `tol`."""
    L, W = geometry
    assert out["consumed"] == ref["consumed"] and len(out["sym"]) == len(ref["sym"]), (out["consumed"], len(out["sym"]), stats)
    rep = check_tiled(out["sym"], ref["sym"], stats, first_exact=W // 4 - 8, tol=tol)
    print(rep)
    assert stats["bad_seams"] == 0, (rep, stats)
    assert rep["pass"], (rep, tol)
    if L == 256:
        assert stats["tiles"] > 256, stats                    # the seam scan crossed a block of 256 tiles
    if reports:
        assert len(out["freq"]) == len(ref["freq"]) == len(out["ss"]) == len(out["mer"]) and len(ref["freq"]) > 15
        d_ss, d_mer = np.max(np.abs(out["ss"] / ref["ss"] - 1)), np.max(np.abs(out["mer"] - ref["mer"]))
        print(dict(max_ss_rel=float(d_ss), max_mer_db=float(d_mer)))
        assert d_ss <= tol["ss_rtol"], d_ss
        assert d_mer <= tol["mer_atol_db"], (d_mer, out["mer"] - ref["mer"])
    return rep


@pytest.mark.parametrize("geometry", tc.GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("name", [c["name"] for c in tc.CASES])
def test_tiled_vs_serial_per_constellation(capi, ctx, refs, monkeypatch, name, geometry):
    """BPSK 1/2, QPSK 1/2 decided by the TABLE, 8PSK 2/3: same counts, tile 0 bit-exact, no unreconciled seam, decisions and costs
    within the case's tolerance, and the FREQ / SS / MER reports with the serial receiver's cadence and within ss_rtol / mer_atol_db
    (for BPSK the estimators count the error along the diagonal only, sdr.h:873-889: the other branch is about 3 dB off)."""
    c = refs[name]
    if c["case"]["cstln"] == capi.QPSK:
        monkeypatch.setenv("LSDR_RX_NO_ARITH", "1")           # read by lsdr_rx_create
    r = tiled_receiver(capi, ctx, c["kw"], c["st"], geometry)
    assert not r.decision_mode()["arithmetic"]
    out = r.run(c["tail"])
    stats = r.tiled_stats()
    r.close()
    assert_tiled_is_serial(out, stats, c["ref"], c["tol"], geometry)


# (constellation, code rate): the receiver side of tests/test_gpu_fec.py's VITERBI_MODES, every constellation once
SHORT_MODES = [(0, 0), (1, 0), (2, 1), (3, 3), (4, 6), (5, 2), (6, 3), (7, 2), (8, 5)]


@pytest.mark.parametrize("cstln,fec", SHORT_MODES)
def test_short_input_is_the_serial_loop_per_constellation(capi, ctx, oracle, monkeypatch, cstln, fec):
    """1000 samples into a new receiver, 1024-sample tiles after 512 of warm-up: tile 1's warm-up starts at the run's first sample
    from the initial state (mu = phase = 0), so the tile kernel — its table slicer for every constellation — retraces the serial
    loop: cost and symbol equal the oracle's bit for bit.  No lock is needed for that, so this holds for the dense constellations too.
    (A tile keeps its frequency within 65536 / omega / 2048 = 8 units of the carried one, which the serial loop does not: the input is
    the constellation's own signal with no carrier offset, on which the serial loop stays within a quarter of that.)"""
    monkeypatch.setenv("LSDR_RX_NO_ARITH", "1")
    x = tc.make_stream(oracle, cstln, fec, 14, 26.0, cfo=0.0, phase0=0.0)[800:1800]
    kw = dict(sampler=1, cstln=cstln, fec=fec, omega=4.0, meas_decimation=4096, pll_adjustment=1.0 if cstln == 1 else 1.0 / 6.0)
    p = po.rx_params(**kw)
    want = oracle.rx(p, x)
    rx, st = tc.SerialRx(oracle, p), oracle.rx(p, x[:1])["state"]
    for k in range(7):
        _, st = rx.run(x[k * tc.CHUNK:(k + 1) * tc.CHUNK + 1], st)
        assert abs(st.freqw) <= 2.0, (k, st.freqw)
    rx.close()
    r = capi.CstlnReceiver(ctx, mode=capi.RX_TILED, tile_len=1024, tile_warmup=512, **kw)
    assert not r.decision_mode()["arithmetic"]
    out = r.run(x)
    stats = r.tiled_stats()
    r.close()
    assert out["consumed"] == want["consumed"] == 896 and stats["tiles"] == 2, stats
    assert len(set(want["sym"]["symbol"])) > (1 << capi.CSTLN_BITS[cstln]) // 2          # (the input reaches the table's regions)
    assert bits_equal(out["sym"]["cost"], want["sym"]["cost"]) and bits_equal(out["sym"]["symbol"], want["sym"]["symbol"])


def _boundaries(oracle, c, geometry, want_rots):
    """Sample offsets (behind the acquisition) at which to cut the stream into runs: ends of tiles which — in the emulation with the
    oracle alone — sit in a stretch of three tiles that all took the rotation asked for, so that the run ends on that rotation."""
    em = tc.emulate_tiles(oracle, po.rx_params(**c["kw"]), c["tail"], c["st"], *geometry)
    rot, spans, cuts, j = em["rot"], em["spans"], [], 2
    for want in want_rots:
        while not (rot[j - 1] == rot[j] == rot[j + 1] == want):
            j += 1
        cuts.append(spans[j][1])
        j += 8
    return cuts


def test_state_carry_and_queued_runs_8psk(capi, ctx, oracle, refs):
    """8PSK, three runs cut where the last tile sits on rotation 5, then on rotation 6 (rx_rotate_back turns the carried phase back by
    rot · 65536 / 8, and the next run's labels are in the serial receiver's frame only if it did): two consecutive runs and three
    synchronous runs add up to the serial receiver's counts and stay within the 8PSK bound across the boundaries; three queued runs
    (lsdr_rx_run_async) equal the synchronous ones bit for bit, symbols and final state."""
    c, geometry = refs["psk8_23"], (512, 512)
    x, ref, p = c["tail"], c["ref"], po.rx_params(**c["kw"])
    b1, b2 = _boundaries(oracle, c, geometry, (5, 6))
    assert 0 < b1 < b2 < len(x) - 4096
    # two consecutive runs; the state carried over the boundary is the serial receiver's, but for loop noise
    r = tiled_receiver(capi, ctx, c["kw"], c["st"], geometry)
    o1 = r.run(x[:b1 + 1], meas=False)
    s1 = r.tiled_stats()
    o2 = r.run(x[b1:], meas=False)
    s2 = r.tiled_stats()
    r.close()
    assert o1["consumed"] == b1 and o1["consumed"] + o2["consumed"] == ref["consumed"]
    want1 = oracle.rx(p, x[:b1 + 1], state_in=c["st"])
    dphi = (o1["state"].phase - want1["state"].phase + 32768.0) % 65536.0 - 32768.0
    assert abs(dphi) < 65536 / 8 / 4, (dphi, o1["state"].phase, want1["state"].phase)      # (one rotation is 8192)
    got = np.concatenate([o1["sym"], o2["sym"]])
    stats = dict(tiles=s1["tiles"] + s2["tiles"], bad_seams=s1["bad_seams"] + s2["bad_seams"], dup=s1["dup"] + s2["dup"], miss=s1["miss"] + s2["miss"])
    rep = check_tiled(got, ref["sym"], stats, tol=TOL_PSK8)
    print(rep)
    assert len(o1["sym"]) == len(want1["sym"]) and rep["pass"], rep
    assert (o2["sym"]["symbol"] == ref["sym"]["symbol"][len(o1["sym"]):]).mean() >= TOL_PSK8["min_equal_decisions"]
    # three synchronous runs and three queued ones
    a = tiled_receiver(capi, ctx, c["kw"], c["st"], geometry)
    b = tiled_receiver(capi, ctx, c["kw"], c["st"], geometry)
    cuts = [0, b1, b2, len(x)]
    d = ctx.upload(x)
    cap = len(x) // 4 + 4096
    o = ctx.alloc(cap * 4)
    sync, pos = [], 0
    for k in range(3):
        res = a.run_dev(d.at(pos * 8), cuts[k + 1] - pos + (1 if k < 2 else 0), o.ptr, cap, meas=False)
        sync.append(ctx.download(o, capi.SOFTSYM, res["produced"]).copy())
        pos += res["consumed"]
        assert pos == (cuts[k + 1] if k < 2 else ref["consumed"])
    outs = [ctx.alloc(cap * 4) for _ in range(3)]
    pos2 = 0
    for k in range(3):
        pos2 += b.run_async(d.at(pos2 * 8), cuts[k + 1] - pos2 + (1 if k < 2 else 0), outs[k].ptr, cap)
    queued = [ctx.download(outs[k], capi.SOFTSYM, b.wait()).copy() for k in range(3)]
    assert pos2 == pos
    sa, sb = a.state().as_dict(), b.state().as_dict()
    a.close(); b.close(); d.free(); o.free()
    for buf in outs:
        buf.free()
    for k in range(3):
        assert len(sync[k]) > 1000 and bits_equal(queued[k], sync[k]), k
    assert sa == sb
    got3 = np.concatenate(sync)
    assert len(got3) == len(ref["sym"])
    # all of it, and what follows each boundary (thousands of symbols each: the bound allows whole symbols there)
    for lo in (0, len(sync[0]), len(sync[0]) + len(sync[1])):
        assert len(got3) - lo > 8000
        assert (got3["symbol"][lo:] == ref["sym"]["symbol"][lo:]).mean() >= TOL_PSK8["min_equal_decisions"], lo


def test_table_path_and_harden_qpsk(capi, ctx, oracle, refs, monkeypatch):
    """QPSK: the tiles decide by arithmetic (a), by the table (b: LSDR_RX_NO_ARITH), by the hardened table (c: harden = 1).  (a) and (b)
    are the serial receiver's under TOL; hardening changes costs only — (c) has (b)'s symbols and final loop state bit for bit and
    sign(b's cost) as its cost.  And the serial mode with harden = 1: the oracle's symbols, the sign of the oracle's costs."""
    c, geometry = refs["qpsk12_table"], (512, 512)

    def run(**more):
        r = tiled_receiver(capi, ctx, c["kw"], c["st"], geometry, **more)
        arith = r.decision_mode()["arithmetic"]
        out = r.run(c["tail"])
        stats = r.tiled_stats()
        r.close()
        return out, stats, arith

    a, sa, arith_a = run()
    monkeypatch.setenv("LSDR_RX_NO_ARITH", "1")
    b, sb, arith_b = run()
    monkeypatch.delenv("LSDR_RX_NO_ARITH")
    h, sh, arith_h = run(harden=1)
    assert arith_a and not arith_b and not arith_h
    assert_tiled_is_serial(a, sa, c["ref"], TOL, geometry)
    assert_tiled_is_serial(b, sb, c["ref"], TOL, geometry)
    assert bits_equal(h["sym"]["symbol"], b["sym"]["symbol"]) and sh == sb
    assert h["state"].as_dict() == b["state"].as_dict()
    assert np.abs(b["sym"]["cost"].astype(np.int32)).min() > 1       # (no cost of the table is its own sign)
    assert bits_equal(h["sym"]["cost"], np.sign(b["sym"]["cost"]).astype(b["sym"]["cost"].dtype))
    # serial mode, hardened
    n = 16384
    want = oracle.rx(po.rx_params(**c["kw"]), c["x"][:n + 1])
    r = capi.CstlnReceiver(ctx, harden=1, **c["kw"])
    out = r.run(c["x"][:n + 1])
    r.close()
    assert out["consumed"] == want["consumed"] == n and bits_equal(out["sym"]["symbol"], want["sym"]["symbol"])
    assert np.abs(want["sym"]["cost"].astype(np.int32)).min() > 1
    assert bits_equal(out["sym"]["cost"], np.sign(want["sym"]["cost"]).astype(want["sym"]["cost"].dtype))


@pytest.mark.parametrize("limits", ["own", "narrow"])
@pytest.mark.parametrize("geometry", tc.GEOMETRIES, ids=GEO_IDS)
def test_allow_drift_and_cfg_freq(capi, ctx, oracle, refs, geometry, limits):
    """A receiver tuned to freq = DRIFT_FREQ with allow_drift = 1 on the stream shifted there, against the serial oracle configured
    alike, under TOL.  "narrow": the carried state's drift limits are ± 8 units around 0, far from the carrier (65.5 units per
    sample) — with allow_drift the reference never looks at them (sdr.h:895-898), and a tile that did would pull its frequency to 0
    at the end of every chunk."""
    c = refs["drift"]
    st, ref = c["st"], c["ref"]
    assert abs(st.freqw - tc.DRIFT_FREQ * 65536) < 8 and st.min_freqw < st.freqw < st.max_freqw
    if limits == "narrow":
        st = tc.copy_state(st, min_freqw=-8.0, max_freqw=8.0)
        ref = oracle.rx(po.rx_params(**c["kw"]), c["tail"], state_in=st)
        assert bits_equal(ref["sym"], c["ref"]["sym"])
    r = tiled_receiver(capi, ctx, c["kw"], st, geometry)
    out = r.run(c["tail"])
    stats = r.tiled_stats()
    r.close()
    assert_tiled_is_serial(out, stats, ref, TOL, geometry)
    # the FREQ report stands at the carrier: DRIFT_FREQ plus the stream's own 3e-5, to a third of the latter
    assert abs(np.mean(out["freq"]) - (tc.DRIFT_FREQ + 3e-5)) < 1e-5 and abs(np.mean(ref["freq"]) - (tc.DRIFT_FREQ + 3e-5)) < 1e-5
