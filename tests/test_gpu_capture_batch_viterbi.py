"""lsdr_capture_batch's Viterbi engine (lsdr_capture_batch_create_viterbi): B independent cu8 captures, each from its first sample to TS by
leandvb's `--viterbi` graph per capture (auto_notch → cstln_receiver(linear, pll_adjustment / 6) → viterbi_sync → mpeg_sync(deconv = NULL) →
deinterleaver → rs_decoder → derandomizer), in shared launches.

  * whole job: every capture's TS against the reference BINARY's for the same IQ (`leandvb --u8 -f 2400e3 --sr 2000e3 --cr 1/2 --viterbi`),
    on captures so noisy that the default graph decodes little or nothing of them, by bench_c1.verify's rule;
  * front end: the soft symbols — costs included — against the oracle's exact chain under leansdr_amd.tolerance.TOL, tile 0 bit for bit;
  * Viterbi stage and tail: given the object's own soft symbols, the bytes are a fresh single-stream lsdr_viterbi_run's, and the rest is
    what the one-block-per-call C ABI produces from those bytes when the host drives it;
  * a capture's TS and its number of Viterbi rounds do not depend on what else is in the batch.

The reference binary (oracle/_ref/leandvb) is required: where it is missing these tests FAIL.
"""
import numpy as np
import pytest
from batch_common import REF_U8, _assert_stages_exact, capture, check_against_reference, decode_batch, references, six_variants

pytestmark = pytest.mark.gpu

REF_ARGS = REF_U8 + ("--viterbi",)
WEAK = [(21, 12), (22, 15), (23, 18), (24, 20)]           # (seed, noise_std): the default graph returns 1446 / 1133 / 4 / 0 packets of 1500


def _decode(capi, ctx, iqs, n_samples, anf, tile, cb=None):
    """One batch on a (new, unless given) Viterbi object: (object, results, TS per capture)."""
    import bench_c1
    return decode_batch(ctx, iqs, n_samples, lambda: capi.CaptureBatch(ctx, len(iqs), n_samples, bench_c1.OMEGA, anf=anf, tile_len=tile, tile_warmup=512,
                                                                       viterbi=True), cb)


@pytest.mark.parametrize("tile", [4096, 2048])
def test_weak_captures_decode_to_the_reference_ts(capi, ctx, tile):
    """B = 4, anf 0, noise 12 … 20: at 18 and 20 the default engine returns nothing."""
    caps = [capture(1500, s, n) for s, n in WEAK]
    n = len(caps[0][0]) // 2
    assert n == 2937623 and all(len(c[0]) == 2 * n for c in caps)
    refs = references([(REF_ARGS + ("--anf", "0"), 1500, s, nz) for s, nz in WEAK])
    cb, res, ts = _decode(capi, ctx, [c[0] for c in caps], n, 0, tile)
    try:
        for i, (s, nz) in enumerate(WEAK):
            check_against_reference(ts[i], refs[i], caps[i][1], 1400, f"seed {s} noise {nz} tile {tile}", False)
            r = res[i]
            assert r["locked"] == 1 and r["seam_bad"] == 0 and r["next_sync_calls"] == 0, r
            st = cb.viterbi_stats(i)
            assert st["bytes"] == r["bytes_deconv"] and st["current_sync"] == r["alignment"] and st["rounds"] >= 1, (st, r)
            assert st["batch_rounds"] >= st["rounds"]
        assert capi.lib.lsdr_capture_batch_words_dev(cb.h, 0) is None
        assert cb.soft_ptr(4) is None and cb.soft_ptr(-1) is None and capi.lib.lsdr_capture_batch_ts_dev(cb.h, 4) is None
    finally:
        cb.close()


def test_across_a_detect_point_with_the_notch(capi, ctx):
    """anf = 1 (leandvb's default), 5.9 M samples: the first detect point is at sample 4 190 208.  Then a short run on the same object."""
    iq, sent = capture(3000, 31, 18)
    n = len(iq) // 2
    assert n == 5875223
    iq23, sent23 = capture(1500, 23, 18)
    ref, ref_short = references([(REF_ARGS, 3000, 31, 18), (REF_ARGS, 1500, 23, 18, 1000000)])
    cb, res, ts = _decode(capi, ctx, [iq, iq], n, 1, 4096)
    try:
        check_against_reference(ts[0], ref, sent, 2900, "seed 31 noise 18 anf 1", False)
        assert ts[0] == ts[1]
        assert all(r["locked"] == 1 and r["seam_bad"] == 0 and r["next_sync_calls"] == 0 for r in res), res
        assert len(cb.bins(0)) == 1
        _, res2, ts2 = _decode(capi, ctx, [iq23, iq23], 1000000, 1, 4096, cb=cb)
        check_against_reference(ts2[0], ref_short, sent23, 400, "seed 23 noise 18, 1 000 000 samples, second run", False)
        assert ts2[0] == ts2[1]
        assert all(r["samples"] == (1000000 // 4096 * 4096 - 1) // 128 * 128 for r in res2), res2
    finally:
        cb.close()


@pytest.mark.parametrize("anf,tile,cw_amp", [(1, 4096, 14.0), (1, 2048, 14.0), (0, 4096, 0.0)])
def test_soft_symbols_against_the_oracle_chain(capi, ctx, oracle, anf, tile, cw_amp):
    """cconverter → auto_notch → cstln_receiver(linear, pll_adjustment 1/6): the batch's soft symbols, costs included, against the oracle's
    sequential exact chain under tolerance.TOL; the symbols of tile 0 bit for bit."""
    import bench_c1
    import pyoracle as po
    from leansdr_amd import tolerance
    n = 1 << 20
    dec_period = 64 * 4096
    gen = bench_c1.Generator(capi, ctx, n, 2)
    caps = []
    for k in range(2):
        d, _ = gen.capture(k, 900 + k)
        iq = ctx.download(d, np.uint8, 2 * n)
        d.free()
        if cw_amp:
            t = np.arange(n)
            f = np.where(t < 2 * dec_period + 4096 * 5, 0.1234, -0.31)
            ph = 2 * np.pi * np.cumsum(f)
            x = iq.reshape(-1, 2).astype(np.float64) - 128 + cw_amp * np.stack([np.cos(ph), np.sin(ph)], axis=1)
            iq = np.clip(np.rint(x + 128), 0, 255).astype(np.uint8).reshape(-1)
        caps.append(iq)
    gen.close()
    bufs = [ctx.upload(c) for c in caps]
    cb = capi.CaptureBatch(ctx, 2, n, bench_c1.OMEGA, anf=anf, tile_len=tile, tile_warmup=512, notch_decimation=dec_period if anf else 0, viterbi=True)
    try:
        cb.run_async([b.ptr for b in bufs], n)
        res = cb.wait()
        for i in range(2):
            xf = oracle.cconverter_u8(caps[i])
            if anf:
                xf, _ = oracle.auto_notch(xf, 1, dec_period)
            o = oracle.rx(po.rx_params(sampler=1, cstln=1, omega=bench_c1.OMEGA, meas_decimation=1 << 20, pll_adjustment=1.0 / 6.0), xf)
            assert res[i]["samples"] == o["consumed"]
            sym = cb.soft(i, res[i]["symbols"])
            assert not sym["pad"].any()
            first = int(512 / bench_c1.OMEGA) - 8
            rep = tolerance.check_tiled(sym, o["sym"], dict(tiles=res[i]["tiles"], bad_seams=res[i]["seam_bad"], dup=res[i]["seam_dup"], miss=res[i]["seam_miss"]),
                                        first_exact=first)
            print(f"anf {anf} tile {tile} capture {i}: {rep}")
            assert rep["pass"], rep
    finally:
        cb.close()
        for b in bufs:
            b.free()


def test_viterbi_stage_and_tail_are_exact_on_the_objects_own_soft_symbols(capi, ctx):
    import bench_c1
    n = 8 << 20
    gen = bench_c1.Generator(capi, ctx, n, 1)
    d0, _ = gen.capture(0, 777)
    gen.close()
    base = ctx.download(d0, np.uint8, 2 * n)
    d0.free()
    variants = six_variants(base, n, 300000)
    names = [v[0] for v in variants]
    bufs = [ctx.upload(v) for _, v in variants]
    cb = capi.CaptureBatch(ctx, len(variants), n, bench_c1.OMEGA, anf=0, tile_len=2048, tile_warmup=512, viterbi=True)
    try:
        res, ts = cb.decode([b.ptr for b in bufs], n)
        _assert_stages_exact(capi, ctx, cb, res, ts, names)
        print("rounds:", [cb.viterbi_stats(i) for i in range(len(variants))])
        assert res[0]["ts_packets"] > 4000 and res[0]["locked"] == 1
        assert all(res[i]["ts_packets"] > 4000 for i in (1, 2, 3))                    # viterbi_sync's alignment search takes the rotation
        assert len({res[i]["alignment"] for i in range(4)}) > 1
        assert 500 < res[4]["ts_packets"] < res[0]["ts_packets"]                      # the burst cost packets, both halves decoded
        assert res[5]["ts_packets"] == 0 and res[5]["locked"] == 0
        # a SHORT run on the same object
        short = base[: 2 * 70000].copy()
        sb = ctx.upload(short)
        res2, ts2 = cb.decode([sb.ptr] * len(variants), len(short) // 2)
        assert all(r["samples"] == (len(short) // 2 - 1) // 128 * 128 for r in res2)
        assert len(set(ts2)) == 1
        _assert_stages_exact(capi, ctx, cb, res2[:2], ts2[:2], ["short run, capture 0", "short run, capture 1"])
        sb.free()
    finally:
        cb.close()
        for b in bufs:
            b.free()


def test_neighbours_do_not_matter(capi, ctx):
    caps = [capture(1500, s, n)[0] for s, n in WEAK]
    n = len(caps[0]) // 2
    cb4, res4, ts4 = _decode(capi, ctx, caps, n, 0, 4096)
    st4 = cb4.viterbi_stats(2)
    cb4.close()
    cb1, res1, ts1 = _decode(capi, ctx, [caps[2]], n, 0, 4096)
    st1 = cb1.viterbi_stats(0)
    cb1.close()
    assert ts1[0] == ts4[2] and len(ts1[0]) > 1400 * 188
    assert st1["rounds"] == st4["rounds"] and st1["symbols"] == st4["symbols"] and st1["bytes"] == st4["bytes"], (st1, st4)
    # the rounds are shared: four copies of a capture take as many as the capture alone
    cbc, resc, tsc = _decode(capi, ctx, [caps[2]] * 4, n, 0, 4096)
    try:
        stc = [cbc.viterbi_stats(i) for i in range(4)]
        assert all(t == ts1[0] for t in tsc)
        assert all(s["rounds"] == st1["rounds"] and s["batch_rounds"] == st1["batch_rounds"] for s in stc), (stc, st1)
    finally:
        cbc.close()


def test_two_partitions_give_the_same_ts(capi, ctx):
    """aux_cus: the tiles on one compute-unit partition, everything else — Viterbi stage and tail included — on the other."""
    import bench_c1
    iq = capture(1500, 23, 18)[0]
    n = len(iq) // 2
    cb0, res0, ts0 = _decode(capi, ctx, [iq, iq], n, 0, 4096)
    cb0.close()
    bufs = [ctx.upload(iq) for _ in range(2)]
    cb = capi.CaptureBatch(ctx, 2, n, bench_c1.OMEGA, anf=0, tile_len=4096, tile_warmup=512, aux_cus=64, viterbi=True)
    try:
        for _ in range(2):                                    # (a second batch on the same object)
            res, ts = cb.decode([b.ptr for b in bufs], n)
            assert ts == ts0 and len(ts[0]) > 1400 * 188
            assert [r["symbols"] for r in res] == [r["symbols"] for r in res0]
    finally:
        cb.close()
        for b in bufs:
            b.free()
