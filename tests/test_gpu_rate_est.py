"""lsdr_rate_est on the GPU: every capture's samples per symbol estimated from its raw samples, and the batch decoders constructed with the
estimate.

  a the device against the float64 restatement (rate_common.estimate) and against the TRUE rate: the twelve captures of the case list
    (6/5 … 12 samples per symbol, noise 7.5 and 18, 0.03 cycles per sample off tune) in one batch;
  b the five sample formats of the same samples give the cu8 record bit for bit;
  c lengths and composition: whole blocks only, all-zero records where there is none, a capture's record does not depend on the batch it
    is in or on its place, two runs are equal, a pointer that is only item-aligned, the longest grid (256 blocks), a capture whose second
    block is all zeros;
  d every refusal is LSDR_E_ARG with a message naming rate_est and leaves a usable object;
  e the loop closed: the 1 958 423-sample captures at 1.2 samples per symbol decoded by CaptureBatch (default and viterbi) and HsBatch
    constructed with the ESTIMATED omega, against `leandvb --sr 2000e3`; a mixed job (6/5 and 3 samples per symbol in one estimator
    batch) grouped by capi.group_by_omega; and, constructed with omega 1.25, the decoders lose more than half the packets.

Bounds: |omega/true − 1| ≤ 2.5e-4 (rate_common.REL: a quarter of the 1e-3 by which the reference's --sr may be off with its TS unchanged);
powers and floor within 1e-4·c of the restatement's (float32 FFT against float64); corr within 1e-5; omega within 1e-6 relative of steps
5 and 6 evaluated in float64 on the device's own powers, floor and corr.
Measured on an MI355X: powers and floor within 3.4e-7·c, corr within 3.6e-8, omega within 4.5e-8 of the formula, max |omega/true − 1|
3.02e-5 (8 samples per symbol, noise 7.5), quality 46.6 … 186.9; the 1 958 423-sample captures give omega 1.2000004 (noise 7.5) and
1.2000006 (noise 18) and every decoder returns the reference's whole TS (946, 932, 956 packets); constructed with omega 1.25 all three
return 0 packets.
The reference binary (oracle/_ref/leandvb) is required by e: where it is missing that test FAILS.
"""
import ctypes as C

import numpy as np
import pytest
import rate_common as rc
from batch_common import REF_U8, capture, check_against_reference, references

pytestmark = pytest.mark.gpu

LSDR_E_ARG = -2
N = rc.N
# the captures of test_gpu_tune_est.py: capture(1000, 11, noise) at 1.2 samples per symbol
N_ALL = 1958423
# decoder → (noise, leandvb's extra arguments, what the reference returns, sent packets asked, from first compared)
DECODERS = {"default": (7.5, ("--anf", "0"), 946, False, False), "viterbi": (18.0, ("--viterbi", "--anf", "0"), 932, True, False),
            "hs": (7.5, ("--hs",), 956, True, True)}
FLOATS = ("omega", "other", "line", "quality", "corr", "floor")


def _same(a, b):
    """Two records bit for bit (floats compared by their bits)."""
    f = lambda r: (np.array([r[k] for k in FLOATS] + r["power"], np.float32).tobytes(), r["bin"], r["blocks"], r["ambiguous"])
    return f(a) == f(b)


def _estimate(capi, ctx, arrays, lengths=None, **kw):
    """One batch of host arrays (None: no pointer), whole or their first lengths[i] items."""
    bufs = [ctx.upload(a) if a is not None else None for a in arrays]
    est = capi.RateEstimator(ctx, len(arrays), **kw)
    try:
        if lengths is None:
            lengths = [len(a) // 2 for a in arrays]
        return est.estimate([b.ptr if b else None for b in bufs], lengths)
    finally:
        est.close()
        for b in bufs:
            if b:
                b.free()


def _formula(g, **kw):
    """Steps 5 and 6 in float64 on the device's own powers, floor and corr."""
    return rc.from_peak(g["bin"], *g["power"], g["floor"], g["corr"], **kw)


# ---- a -----------------------------------------------------------------------------------------------------------------------------
def test_against_the_restatement_and_the_truth(capi, ctx):
    cases = rc.cases()
    got = _estimate(capi, ctx, [iq for _, _, iq in cases])
    d_pow = d_corr = d_omega = d_true = 0.0
    quals = []
    for (name, omega, iq), g in zip(cases, got):
        w = rc.estimate(rc.to_complex(iq))
        assert g["blocks"] == 64 and g["bin"] == w["bin"] and g["ambiguous"] == w["ambiguous"] == 0, (name, g, w)
        assert rc.chose_a(g) == rc.chose_a(w) == (omega >= 2), (name, g, w)
        c = w["power"][1]
        dp = max(abs(a - b) for a, b in zip(g["power"] + [g["floor"]], w["power"] + [w["floor"]])) / c
        dc = abs(g["corr"] - w["corr"])
        f = _formula(g)
        do = max(abs(g["omega"] / f["omega"] - 1), abs(g["other"] / f["other"] - 1), abs(g["line"] / f["line"] - 1))
        dt = abs(g["omega"] / omega - 1)
        d_pow, d_corr, d_omega, d_true = max(d_pow, dp), max(d_corr, dc), max(d_omega, do), max(d_true, dt)
        quals.append(g["quality"])
        print(f"{name}: omega {g['omega']:.6f} off by {dt:.2e}, quality {g['quality']:.1f}, corr {g['corr']:.4f}, powers {dp:.1e} of c, corr {dc:.1e}")
        assert dp <= 1e-4, (name, dp)
        assert dc <= 1e-5, (name, dc)
        assert do <= 1e-6, (name, do)
        assert dt <= rc.REL, (name, g["omega"])
        assert g["quality"] == pytest.approx(g["power"][1] / g["floor"], rel=1e-6)
    print(f"device against the restatement: powers within {d_pow:.2e} of c, corr within {d_corr:.2e}, omega within {d_omega:.2e} of the "
          f"formula; max |omega/true - 1| {d_true:.3e} (bound {rc.REL:.1e}); quality {min(quals):.1f} ... {max(quals):.1f}")


# ---- b -----------------------------------------------------------------------------------------------------------------------------
def test_formats_give_the_same_record(capi, ctx):
    u8 = rc.shifted_capture(3, 2, 18.0, 8)
    s8 = (u8.astype(np.int16) - 128).astype(np.int8)
    s16 = (s8.astype(np.int16) * 256).astype(np.int16)
    u16 = (s16.astype(np.int32) + 32768).astype(np.uint16)
    f32 = s8.astype(np.float32)
    base = _estimate(capi, ctx, [u8])[0]
    assert base["blocks"] == 8 and abs(base["omega"] / 1.5 - 1) <= 4 * rc.REL and base["quality"] >= capi.RATE_MIN_QUALITY, base
    for name, items, kw in (("cs8", s8, dict(in_format=capi.IN_CS8)), ("cs16 scaled", s16, dict(in_format=capi.IN_CS16, in_scale=2.0 ** -8)),
                            ("cu16 scaled", u16, dict(in_format=capi.IN_CU16, in_scale=2.0 ** -8)),
                            ("cf32", f32, dict(in_format=capi.IN_CF32, in_scale=1.0)), ("cu8 scale 1", u8, dict(in_scale=1.0))):
        got = _estimate(capi, ctx, [items], **kw)[0]
        assert _same(got, base), (name, got, base)
    raw = _estimate(capi, ctx, [s16], in_format=capi.IN_CS16)[0]           # 256 times larger: the normalisation takes it
    assert np.isfinite(raw["quality"]) and raw["bin"] == base["bin"] and abs(raw["omega"] / base["omega"] - 1) <= 1e-6, (raw, base)


# ---- c -----------------------------------------------------------------------------------------------------------------------------
def test_composition_and_lengths(capi, ctx):
    iq = rc.shifted_capture(6, 5, 7.5, 65)
    lengths = [64 * N, 64 * N + 4095, N, N - 1, 0, 3 * N + 1]
    B = len(lengths)
    buf = ctx.upload(iq)
    ptrs = [buf.ptr if n else None for n in lengths]
    est = capi.RateEstimator(ctx, B)
    one = capi.RateEstimator(ctx, 1)
    try:
        got = est.estimate(ptrs, lengths)
        for g, n in zip(got, lengths):                                      # every one is the restatement's
            w = rc.estimate(rc.to_complex(iq[: 2 * n]))
            assert g["blocks"] == w["blocks"] and g["bin"] == w["bin"] and abs(g["power"][1] - w["power"][1]) <= 1e-4 * max(w["power"][1], 1.0), (n, g, w)
            assert rc.chose_a(g) == rc.chose_a(w) or not w["blocks"], (n, g, w)
        assert [g["blocks"] for g in got] == [64, 64, 1, 0, 0, 3]
        assert got[3] == rc.ZERO and got[4] == rc.ZERO
        assert _same(got[0], got[1]) and not _same(got[0], got[5])
        again = est.estimate(ptrs, lengths)
        assert all(_same(a, b) for a, b in zip(got, again))
        back = est.estimate(ptrs[::-1], lengths[::-1])
        assert all(_same(a, b) for a, b in zip(got, back[::-1]))
        for i, n in enumerate(lengths):
            alone = one.estimate([ptrs[i]], [n])[0]
            assert _same(alone, got[i]), (n, alone, got[i])
        # a pointer that is item-aligned only (the item-wise loads): the same samples give the same record
        moved = ctx.upload(np.concatenate([np.zeros(2, np.uint8), iq]))
        try:
            assert _same(one.estimate([moved.at(2)], [64 * N])[0], got[0])
        finally:
            moved.free()
    finally:
        est.close()
        one.close()
        buf.free()


def test_the_longest_grid_and_an_all_zero_block(capi, ctx):
    long_iq = rc.shifted_capture(4, 1, 18.0, 256)
    holed = long_iq[: 2 * 3 * N].copy()
    holed[2 * N: 4 * N] = 128                                               # cu8: the second block is all zeros
    got = _estimate(capi, ctx, [long_iq, long_iq, holed], [256 * N, N, 3 * N], blocks=256)
    want = [rc.estimate(rc.to_complex(long_iq), 256), rc.estimate(rc.to_complex(long_iq[: 2 * N]), 256), rc.estimate(rc.to_complex(holed), 256)]
    assert [g["blocks"] for g in got] == [256, 1, 3] == [w["blocks"] for w in want]
    for g, w in zip(got, want):
        assert g["bin"] == w["bin"] and abs(g["power"][1] - w["power"][1]) <= 1e-4 * w["power"][1] and abs(g["corr"] - w["corr"]) <= 1e-5, (g, w)
        assert abs(g["omega"] / _formula(g)["omega"] - 1) <= 1e-6
    assert abs(got[0]["omega"] / 4.0 - 1) <= rc.REL, got[0]
    # the hole is not counted: the capture's first and third block alone give the same powers and corr
    two = _estimate(capi, ctx, [np.concatenate([holed[: 2 * N], holed[4 * N:]])])[0]
    assert two["blocks"] == 2 and two["power"] == got[2]["power"] and two["corr"] == got[2]["corr"] and two["omega"] == got[2]["omega"], (two, got[2])
    print(f"256 blocks: omega off by {abs(got[0]['omega'] / 4.0 - 1):.2e}, quality {got[0]['quality']:.1f}; one block: omega {got[1]['omega']:.5f}, "
          f"quality {got[1]['quality']:.1f}; a hole: omega {got[2]['omega']:.5f}, quality {got[2]['quality']:.1f}")


def test_the_admissible_range(capi, ctx):
    iq = rc.shifted_capture(6, 5, 7.5, 8)
    both = _estimate(capi, ctx, [iq])[0]
    only_a = _estimate(capi, ctx, [iq], omega_min=2.5)[0]
    only_b = _estimate(capi, ctx, [iq], omega_max=1.9)[0]
    none = _estimate(capi, ctx, [iq], omega_min=7.0, omega_max=8.0)[0]
    assert abs(both["omega"] / 1.2 - 1) <= 4 * rc.REL and abs(both["other"] / 6.0 - 1) <= 20 * rc.REL and both["bin"] == 683, both
    assert only_a["omega"] == both["other"] and only_a["other"] == 0.0 and only_a["power"] == both["power"], (only_a, both)
    assert only_b["bin"] == 683 and only_b["other"] == 0.0 and abs(only_b["omega"] / _formula(only_b, omega_max=1.9)["omega"] - 1) <= 1e-6, only_b
    assert none == rc.ZERO
    for g, kw in ((only_a, dict(omega_min=2.5)), (only_b, dict(omega_max=1.9))):
        w = rc.estimate(rc.to_complex(iq), **kw)
        assert g["bin"] == w["bin"] and abs(g["floor"] - w["floor"]) <= 1e-4 * w["power"][1] and g["omega"] == pytest.approx(w["omega"], rel=1e-5), (g, w)


# ---- d -----------------------------------------------------------------------------------------------------------------------------
def test_arguments(capi, ctx):
    lib = capi.lib
    iq = rc.shifted_capture(6, 5, 7.5, 8)
    buf = ctx.upload(iq)
    est = capi.RateEstimator(ctx, 2)
    want = None

    def usable():
        nonlocal want
        got = est.estimate([buf.ptr, None], [8 * N, 0])
        assert got[0]["blocks"] == 8 and got[1] == rc.ZERO and abs(got[0]["omega"] / 1.2 - 1) <= 4 * rc.REL, got
        want = want or got
        assert all(_same(a, b) for a, b in zip(got, want))

    def message(rc_, what):
        msg = lib.lsdr_last_error().decode()
        assert rc_ == LSDR_E_ARG and "rate_est" in msg, (what, rc_, msg)
        return msg

    try:
        usable()
        for what, word, change in (("n_captures 0", "n_captures", lambda c: setattr(c, "n_captures", 0)),
                                   ("n_captures -1", "n_captures", lambda c: setattr(c, "n_captures", -1)),
                                   ("format 5", "in_format", lambda c: setattr(c, "in_format", 5)),
                                   ("format -1", "in_format", lambda c: setattr(c, "in_format", -1)),
                                   ("scale -1", "in_scale", lambda c: setattr(c, "in_scale", -1.0)),
                                   ("scale nan", "in_scale", lambda c: setattr(c, "in_scale", float("nan"))),
                                   ("scale inf", "in_scale", lambda c: setattr(c, "in_scale", float("inf"))),
                                   ("blocks 257", "blocks", lambda c: setattr(c, "blocks", 257)),
                                   ("omega_min 1.0", "omega_min", lambda c: setattr(c, "omega_min", 1.0)),
                                   ("omega_min -2", "omega_min", lambda c: setattr(c, "omega_min", -2.0)),
                                   ("omega_min nan", "omega_min", lambda c: setattr(c, "omega_min", float("nan"))),
                                   ("omega_max 65", "omega_max", lambda c: setattr(c, "omega_max", 65.0)),
                                   ("omega_max 1.0", "omega_max", lambda c: setattr(c, "omega_max", 1.0)),
                                   ("omega_max inf", "omega_max", lambda c: setattr(c, "omega_max", float("inf"))),
                                   ("reversed", "above", lambda c: (setattr(c, "omega_min", 4.0), setattr(c, "omega_max", 3.0))),
                                   ("reserved", "reserved", lambda c: c.reserved.__setitem__(1, 1))):
            cfg = capi.RateEstCfg()
            cfg.n_captures, cfg.in_format, cfg.in_scale, cfg.blocks = 2, capi.IN_CU8, 0.0, 8
            change(cfg)
            h = C.c_void_p()
            assert word in message(lib.lsdr_rate_est_create(ctx.h, C.byref(cfg), C.byref(h)), what) and not h.value
            usable()
        ptrs, lens = est._args([buf.ptr, None], [8 * N, 0])
        assert "in flight" in message(lib.lsdr_rate_est_wait(est.h, est._out), "wait with nothing in flight")
        usable()
        est.run_async([buf.ptr, None], [8 * N, 0])
        assert "in flight" in message(lib.lsdr_rate_est_run_async(est.h, ptrs, lens), "a second run_async before wait")
        assert all(_same(a, b) for a, b in zip(est.wait(), want))
        usable()
        bad, _ = est._args([buf.ptr + 1, None], [8 * N, 0])
        assert "aligned" in message(lib.lsdr_rate_est_run_async(est.h, bad, lens), "a misaligned pointer")
        usable()
        bad, lens1 = est._args([buf.ptr, None], [8 * N, N])
        assert "pointer" in message(lib.lsdr_rate_est_run_async(est.h, bad, lens1), "samples without a pointer")
        usable()
        # cf32 items want 8 bytes
        e32 = capi.RateEstimator(ctx, 1, in_format=capi.IN_CF32)
        try:
            p, n1 = e32._args([buf.ptr + 4], [N])
            assert "aligned" in message(lib.lsdr_rate_est_run_async(e32.h, p, n1), "cf32 at 4 bytes")
        finally:
            e32.close()
        usable()
    finally:
        est.close()
        buf.free()


# ---- e -----------------------------------------------------------------------------------------------------------------------------
def _make(capi, ctx, decoder, n, omega):
    if decoder == "hs":
        return capi.HsBatch(ctx, n, N_ALL, omega, fastlock=0)
    return capi.CaptureBatch(ctx, n, N_ALL, omega, anf=0, tile_len=4096, tile_warmup=512, viterbi=decoder == "viterbi")


@pytest.mark.parametrize("decoder", ["default", "viterbi", "hs"])
def test_the_loop_closed(capi, ctx, decoder):
    noise, extra, ref_packets, ask_sent, from_first = DECODERS[decoder]
    iq, sent = capture(1000, 11, noise)
    assert len(iq) == 2 * N_ALL
    ref = references([(REF_U8 + extra, 1000, 11, noise, None, 0.0)])[0]
    buf = ctx.upload(iq)
    try:
        e = _estimate(capi, ctx, [iq])[0]                                   # the rate NOT given
        assert e["blocks"] == 64 and e["quality"] >= capi.RATE_MIN_QUALITY and not e["ambiguous"] and abs(e["omega"] / 1.2 - 1) <= rc.REL, e
        (omega, members), = capi.group_by_omega([e])[0]
        assert members == [0] and omega == e["omega"]
        print(f"{decoder}: estimated omega {omega:.7f} (off by {abs(omega / 1.2 - 1):.2e}), quality {e['quality']:.1f}, corr {e['corr']:.3f}")
        obj = _make(capi, ctx, decoder, 1, omega)
        try:
            res, ts = obj.decode([buf.ptr], N_ALL)
        finally:
            obj.close()
        check_against_reference(ts[0], ref, sent if ask_sent else None, ref_packets - 10, f"{decoder} omega estimated", from_first)
        assert res[0]["locked"] == 1 and res[0]["seam_bad"] == 0, res[0]
        # the test has teeth: constructed with omega 1.25, the decoder loses the capture
        off = _make(capi, ctx, decoder, 1, 1.25)
        try:
            res0, ts0 = off.decode([buf.ptr], N_ALL)
        finally:
            off.close()
        print(f"{decoder}: decoded with omega 1.25: {len(ts0[0]) // 188} packets (reference, --sr 2000e3: {len(ref) // 188})")
        assert len(ts0[0]) // 188 < len(ref) // 188 // 2
    finally:
        buf.free()


def test_a_mixed_job_is_grouped_by_rate(capi, ctx):
    job = [rc.shifted_capture(6, 5, 7.5), rc.shifted_capture(3, 1, 7.5), rc.shifted_capture(6, 5, 18.0), rc.shifted_capture(3, 1, 18.0)]
    noise = np.clip(np.rint(np.random.default_rng(3).normal(0.0, 30.0, 2 * N * 64) + 128), 0, 255).astype(np.uint8)
    est = _estimate(capi, ctx, job + [noise])
    groups, left = capi.group_by_omega(est)
    assert left == [4] and est[4]["quality"] < capi.RATE_MIN_QUALITY, est[4]
    assert [g[1] for g in groups] == [[0, 2], [1, 3]], groups
    assert abs(groups[0][0] / 1.2 - 1) <= rc.REL and abs(groups[1][0] / 3.0 - 1) <= rc.REL, groups
    print(f"mixed job: groups {groups}, noise-only quality {est[4]['quality']:.2f}")
