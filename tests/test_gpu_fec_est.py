"""lsdr_fec_est on the GPU: every stream's code rate estimated from its hard symbols, and the batch decoders' decisions scored.

  a counts bit for bit: every field of every record, all five `score` entries included, equals the numpy restatement of the definition
    (fec_est_common.estimate) — on random symbols and on the 3/4 capture's oracle decisions, in the three input formats, at the lengths
    where the word tail, the first refill, the skip bound and the tile seam can go wrong (0, 31, 32, 33, 35, 36, 47, 4096, 4097, one tile,
    one tile + 1, three tiles + 17), packed streams starting 0, 5 and 16 symbols into their first word.  Every stream is a prefix of a
    longer buffer: what lies behind symbol n − 1 is there and must not count.  The byte and soft formats carry garbage above `symbol & 3`;
  b the same record alone, in any batch, at any place of it and in every format; max_symbols smaller than n scores exactly the prefix;
  c decisions: the five captures (code rates 1/2 … 7/8, 1.2 samples per symbol, noise 7.5) and a noise-only one as cu8 through
    CaptureBatch(fec=FEC12), its Viterbi engine (soft symbols) and HsBatch, one uniform batch each (padded with their own leading samples to equal length; the original symbol
    count is scored): estimate_fec returns the transmitted rate, locked, not ambiguous; the noise comes back not locked.  The tiled
    receivers' decisions are tolerance-class, so only the decision is asserted; the fractions are printed (and written to the file
    LSDR_FEC_ACCURACY_LOG names: profiles/fec_estimate/accuracy.txt).  The rate-1/2 capture, grouped by capi.group_by_fec and decoded by
    CaptureBatch(fec=FEC12), returns only transmitted packets (16 packets are too few for mpeg_sync: it returns none); the loop is
    closed on the 1000-packet capture of the other batch tests — made with fec 7/8 the object returns next to nothing, its decisions
    say 1/2, and the object made with that returns the transmitted packets;
  d every refusal is LSDR_E_ARG with a message naming fec_est and leaves a usable object.

Measured on an MI355X (profiles/fec_estimate/accuracy.txt): capture batch 0.044 / 0.058 / 0.081 / 0.099 / 0.135 for the transmitted
rates 1/2 … 7/8 and at least 0.468 for every other; its Viterbi engine 0.042 / 0.056 / 0.074 / 0.096 / 0.129 and at least 0.470; hs batch
0.067 / 0.073 / 0.112 / 0.143 / 0.160 and at least 0.470; noise only 0.480, 0.475 and 0.481.  The 1000-packet capture: 0.000 beside
0.300 over 16384 symbols (ambiguous), 0.000 beside 0.471 over 131072; made with 7/8 0 packets, made with the estimate 946.  The whole
file takes 2 s.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import fec_est_common as fc

pytestmark = pytest.mark.gpu

BIG = 1 << 20


def _lengths(tile):
    return [0, 31, 32, 33, 35, 36, 47, 4096, 4097, tile, tile + 1, 3 * tile + 17]


@functools.lru_cache(maxsize=None)
def _source(name, n):
    if name == "random":
        return np.random.default_rng(21).integers(0, 4, n).astype(np.uint8)
    return fc.decisions(3)


@functools.lru_cache(maxsize=None)
def _want(name, total, n, max_symbols=None):
    return fc.estimate(_source(name, total)[:n], max_symbols)


def _image(capi, sym, fmt, off):
    """The host image of a stream in one input format, `off` symbols of other content in front of it."""
    rng = np.random.default_rng(len(sym) + 7 * off + fmt)
    if fmt == capi.HSYM_PACKED2:
        lead = rng.integers(0, 4, off).astype(np.uint8)
        return capi.hs2_pack(np.concatenate([lead, sym]))
    dirty = np.concatenate([rng.integers(0, 256, off).astype(np.uint8), sym | (rng.integers(0, 64, len(sym)).astype(np.uint8) << 2)])
    if fmt == capi.HSYM_U8:
        return dirty
    soft = np.zeros(len(dirty), capi.SOFTSYM)
    soft["symbol"], soft["cost"], soft["pad"] = dirty, rng.integers(-3000, 3000, len(dirty)), rng.integers(0, 256, len(dirty))
    return soft


def _estimate(capi, ctx, fmt, streams, off=0, max_symbols=BIG, est=None):
    """One batch: streams = [(host symbols or None, n)], every one `off` symbols into its buffer."""
    bufs = [ctx.upload(_image(capi, s, fmt, off)) if s is not None else None for s, _ in streams]
    own = est is None
    if own:
        est = capi.FecEstimator(ctx, len(streams), max_symbols, fmt)
    try:
        return est.estimate([b.ptr if b else None for b in bufs], [n for _, n in streams], [off] * len(streams) if off else None)
    finally:
        if own:
            est.close()
        for b in bufs:
            if b:
                b.free()


def _formats(capi):
    return (("packed", capi.HSYM_PACKED2, (0, 5, 16)), ("u8", capi.HSYM_U8, (0, 5)), ("soft", capi.HSYM_SOFT, (0, 3)))


# ---- a -----------------------------------------------------------------------------------------------------------------------------
def test_counts_bit_for_bit(capi, ctx):
    probe = capi.FecEstimator(ctx, 1)
    tile = probe.tile
    probe.close()
    assert tile % 48 == 0 and tile >= 48
    total = 3 * tile + 17
    rnd, cap = _source("random", total), _source("capture", 0)
    assert len(cap) > 4097
    cases = [("random", total, n) for n in _lengths(tile)] + [("capture", 0, n) for n in _lengths(tile) if n <= len(cap)] + [("capture", 0, len(cap))]
    for fname, fmt, offs in _formats(capi):
        for off in offs:
            got = _estimate(capi, ctx, fmt, [((rnd if name == "random" else cap) if n else None, n) for name, _, n in cases], off)
            for (name, tot, n), g in zip(cases, got):
                w = _want(name, tot, n)
                assert g == w, f"{fname}, offset {off}, {name} symbols, n = {n}:\n device {g}\n wanted {w}"
    full = _want("capture", 0, len(cap))
    assert full["fec"] == capi.FEC34 and full["locked"] == 1 and _want("random", total, total)["locked"] == 0    # the inputs are what they are meant to be
    assert _want("random", total, 31)["fec"] == -1 and _want("random", total, 32)["fec"] >= 0


# ---- b -----------------------------------------------------------------------------------------------------------------------------
def test_alone_in_any_batch_and_in_every_format(capi, ctx):
    probe = capi.FecEstimator(ctx, 1)
    tile = probe.tile
    probe.close()
    total = 3 * tile + 17
    rnd = _source("random", total + 128)
    lengths = [0, 5000, 33, 0, total, tile, 4097, 700]
    # different symbols per stream: stream i starts i·11 symbols into the source
    streams = [(rnd[11 * i: 11 * i + n].copy() if n else None, n) for i, n in enumerate(lengths)]
    want = [fc.estimate(s if s is not None else rnd[:0]) for s, _ in streams]
    order = np.random.default_rng(4).permutation(len(streams))
    for fname, fmt, offs in _formats(capi):
        got = _estimate(capi, ctx, fmt, streams, offs[1])
        assert got == want, fname
        shuffled = _estimate(capi, ctx, fmt, [streams[i] for i in order], offs[1])
        assert shuffled == [want[i] for i in order], fname
        one = capi.FecEstimator(ctx, 1, BIG, fmt)
        try:
            for i, s in enumerate(streams):
                assert _estimate(capi, ctx, fmt, [s], est=one) == [want[i]], (fname, i)
        finally:
            one.close()
        short = _estimate(capi, ctx, fmt, streams, max_symbols=1000)
        for (s, n), g in zip(streams, short):
            assert g == fc.estimate(s[:1000] if s is not None else rnd[:0]) and g["symbols"] == min(n, 1000) * (n >= 32), (fname, n)


# ---- c -----------------------------------------------------------------------------------------------------------------------------
def _padded_captures():
    """The five captures and a noise-only one, each repeated from its own start up to the longest's length: (names, IQ arrays, samples,
    original symbol counts)."""
    iqs = [fc.capture(r)[0] for r in fc.RATES]
    n = max(len(iq) for iq in iqs) // 2
    iqs.append(np.random.default_rng(5).integers(96, 160, 2 * n, dtype=np.uint8))
    out = [np.concatenate([iq, iq[: 2 * n - len(iq)]]) for iq in iqs]
    syms = [len(fc.decisions(r)) for r in fc.RATES] + [len(fc.decisions(0))]
    return [fc.NAMES[r] for r in fc.RATES] + ["noise only"], out, n, syms


def _score_batch(ctx, obj, iqs, n, syms):
    bufs = [ctx.upload(iq) for iq in iqs]
    try:
        obj.run_async([b.ptr for b in bufs], n)
        res = obj.wait()
        for r, s in zip(res, syms):
            assert r["symbols"] >= 4096, (r["symbols"], s)                 # condition on the input: the front end ran over the capture
            r["symbols"] = min(r["symbols"], s)
        return obj.estimate_fec(res)
    finally:
        for b in bufs:
            b.free()


def test_decisions_of_both_batch_decoders(capi, ctx):
    names, iqs, n, syms = _padded_captures()
    lines = []
    for what, make in (("capture batch", lambda: capi.CaptureBatch(ctx, len(iqs), n, 1.2, fec=capi.FEC12)),
                       ("capture batch viterbi", lambda: capi.CaptureBatch(ctx, len(iqs), n, 1.2, fec=capi.FEC12, viterbi=True)),   # soft symbols
                       ("hs batch", lambda: capi.HsBatch(ctx, len(iqs), n, 1.2))):
        obj = make()
        try:
            est = _score_batch(ctx, obj, iqs, n, syms)
            again = _score_batch(ctx, obj, iqs, n, syms)                   # the estimator object is kept, and the run repeats
        finally:
            obj.close()
        assert est == again, what
        for name, e in zip(names, est):
            lines.append(f"{what}, {name}: {e['symbols']} symbols, fec {e['fec']}, locked {e['locked']}, ambiguous {e['ambiguous']}, sync {e['sync']}, "
                         f"skip {e['skip']}, E/C per rate " + " ".join(f"{f:.3f}" for f in fc.fractions(e)))
            print(lines[-1])
        for r, e in zip(fc.RATES, est):
            assert e["fec"] == r and e["locked"] == 1 and e["ambiguous"] == 0, (what, fc.NAMES[r], e)
        assert est[-1]["locked"] == 0 and est[-1]["ambiguous"] == 0, (what, est[-1])
        groups, left = capi.group_by_fec(est)
        assert groups == [(r, [i]) for i, r in enumerate(fc.RATES)] and left == [len(iqs) - 1], (what, groups, left)
    log = os.environ.get("LSDR_FEC_ACCURACY_LOG")
    if log:
        with open(log, "w") as f:
            f.write("tests/test_gpu_fec_est.py::test_decisions_of_both_batch_decoders: the disagreement fractions of the tiled receivers' decisions\n"
                    "(five captures of 16 packets at 1.2 samples per symbol, noise 7.5 per component on the cu8 scale, and uniform noise alone)\n")
            f.write("\n".join(lines) + "\n")
    # the loop closed for the rate-1/2 capture: its group's decoder returns only transmitted packets
    (fec, members), = [g for g in groups if g[0] == capi.FEC12]
    iq, sent = fc.capture(fec)
    buf = ctx.upload(iq)
    cb = capi.CaptureBatch(ctx, len(members), len(iq) // 2, 1.2, fec=fec)
    try:
        res, ts = cb.decode([buf.ptr], len(iq) // 2)
    finally:
        cb.close()
        buf.free()
    pk = [ts[0][i:i + 188] for i in range(0, len(ts[0]), 188)]
    print(f"rate 1/2 capture decoded at the estimated rate: {len(pk)} packets")
    assert len(ts[0]) % 188 == 0 and all(p in sent for p in pk)


# synth_dvbs.interleave starts from a pipeline filled with zeros: the first 17·12·11 = 2244 bytes of that generator's code stream — 17952
# symbols at rate 1/2, more than the default 16384 — are half zeros, a stream on which the checks of EVERY rate are satisfied more often
# than by chance (measured: 0.300 for 2/3 beside 0.000 for 1/2, flagged `ambiguous` as it should be).  A recording does not start there;
# this capture is scored over eight times the default instead.
SYMBOLS_PAST_THE_FILL = 131072


def test_a_capture_made_with_the_wrong_rate_is_put_right(capi, ctx):
    """The 16-packet captures above are too short for mpeg_sync to lock.  The loop closed on the 1000-packet rate-1/2 capture of the
    other batch tests (the reference returns 946 packets for it): an object constructed with fec 7/8 returns next to nothing, its
    decisions say 1/2, and the object made with that returns the transmitted packets."""
    from batch_common import capture
    iq, sent = capture(1000, 11, 7.5)
    n = len(iq) // 2
    buf = ctx.upload(iq)
    try:
        wrong = capi.CaptureBatch(ctx, 1, n, 1.2, fec=capi.FEC78)
        try:
            res, ts = wrong.decode([buf.ptr], n)
            head = wrong.estimate_fec(res)
            est = wrong.estimate_fec(res, max_symbols=SYMBOLS_PAST_THE_FILL)
        finally:
            wrong.close()
        print(f"made with 7/8: {res[0]['ts_packets']} packets; first 16384 symbols {head[0]}\nfirst {SYMBOLS_PAST_THE_FILL}: {est[0]}")
        assert head[0]["fec"] == capi.FEC12 and head[0]["locked"] == 1 and head[0]["symbols"] == 16384, head[0]
        assert est[0]["fec"] == capi.FEC12 and est[0]["locked"] == 1 and est[0]["ambiguous"] == 0 and est[0]["symbols"] == SYMBOLS_PAST_THE_FILL, est[0]
        assert est[0]["error_rate"] <= 0.2 and est[0]["runner_up"] >= 0.4, est[0]
        groups, left = capi.group_by_fec(est)
        assert groups == [(capi.FEC12, [0])] and left == []
        right = capi.CaptureBatch(ctx, 1, n, 1.2, fec=groups[0][0])
        try:
            res2, ts2 = right.decode([buf.ptr], n)
        finally:
            right.close()
    finally:
        buf.free()
    pk = [ts2[0][i:i + 188] for i in range(0, len(ts2[0]), 188)]
    good = sum(p in sent for p in pk)
    print(f"made with the estimate: {len(pk)} packets, {good} of them transmitted ones")
    # bench_c1.verify's rule: the default graph's first packets include some of the reference's own acquisition, the first 16 are not asked
    assert len(pk) > 900 and all(p in sent for p in pk[16:])
    assert 2 * res[0]["ts_packets"] < len(pk)                              # made with 7/8, more than half the packets are lost


# ---- d -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_object_usable(capi, ctx):
    def refused(**kw):
        cfg = capi.FecEstCfg()
        cfg.n_streams, cfg.max_symbols, cfg.in_format = kw.get("n_streams", 2), kw.get("max_symbols", 4096), kw.get("in_format", 0)
        cfg.reserved[3] = kw.get("reserved", 0)
        h = C.c_void_p()
        rc = capi.lib.lsdr_fec_est_create(ctx.h, C.byref(cfg), C.byref(h))
        assert rc == -2 and not h and b"fec_est" in capi.lib.lsdr_last_error(), (kw, rc, capi.lib.lsdr_last_error())
    refused(n_streams=0); refused(n_streams=-3); refused(max_symbols=0); refused(in_format=3); refused(in_format=-1); refused(reserved=1)

    sym = _source("random", 5000)
    want = fc.estimate(sym[:4096])
    buf = ctx.upload(capi.hs2_pack(sym))
    est = capi.FecEstimator(ctx, 2, 4096)
    try:
        def fails(call):
            with pytest.raises(capi.LsdrError, match="fec_est"):
                call()
        fails(est.wait)                                                                        # nothing in flight
        fails(lambda: est.run_async([buf.at(2), buf.ptr], [100, 100]))                         # a packed pointer that is not 4-byte aligned
        fails(lambda: est.run_async([None, buf.ptr], [100, 100]))                              # symbols without a pointer
        fails(est.wait)                                                                        # … and nothing was queued
        est.run_async([buf.ptr, None], [5000, 0])
        fails(lambda: est.run_async([buf.ptr, None], [5000, 0]))                               # a run in flight
        got = est.wait()
        assert got[0] == want and got[1]["fec"] == -1 and got[1]["symbols"] == 0
        fails(est.wait)
        assert est.estimate([buf.ptr, buf.ptr], [5000, 4096]) == [want, want]
    finally:
        est.close()
        buf.free()
