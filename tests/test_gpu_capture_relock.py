"""lsdr_capture_batch with re-acquisition (lsdr_capture_relock_set): the device FEC tail keeps the deconvolver one window ahead of
mpeg_sync until the (relocks+1)-th lock, so a next_sync() asked for after a lost lock still takes effect.

The checker is relock_common.chain_gpu — the loop that defines the feature, driven by the host through the one-block-per-call C ABI on
the object's own packed decisions; with relocks = 0 it is batch_common._chain_reference.  Captures: batch_common.rate_capture (the oracle's
leandvbtx | leanchansim, 1.2 samples per symbol) with bursts behind which the carrier comes back turned (relock_common.step_capture).

  1 exactness: rate 1/2, 1200 packets, one batch of eight with relock = 3 — deconvolved bytes, mpeg bytes, TS, every count and the stats
    record equal the chain's bit for bit; no capture is exhausted (asserted on the inputs: no chain locks more than four times);
  2 the cap: relock = 1 equals chain_gpu(relocks = 1) with its `exhausted`; relock = 0, and an object never given the call, equal
    _chain_reference and each other;
  3 the gain: one of the four single steps at least ends locked with more TS packets under relock = 3 than under relock = 0, where it
    ends unlocked; the packets it returns were transmitted (relock_common.assert_transmitted has the rule and why it is not "all");
  4 a capture alone, at another position, after another batch and after relock_set changed: the same record, stats and TS
    (decode_each, ragged lengths with a 0, a tune per capture);
  5 3/4 and 7/8, 2500 packets, a step of 180 degrees: exact against the chain, and the end of the TS is the reference binary's;
  6 a cs16 object gives the cu8 object's TS; unlocked_window = 2048 is exact against its chain;
  7 refusals: a Viterbi object, relocks = 17, a batch in flight, stats before a wait.

Measured on an MI355X: 549 -> 927 / 927 / 911 packets for the steps of 90, 180 and 270 degrees (the step of 0 comes back by itself: 1063), two steps
1023, three steps 639 with four locks; 3/4 1627 packets (reference 2307), 7/8 1107 (1123).  The nine tests take 2.5 s.  The reference binary
(oracle/_ref/leandvb) is required by test 5: where it is missing it FAILS.
"""
import ctypes as C

import numpy as np
import pytest
import relock_common as rc
from batch_common import _chain_reference, packets, rate_capture, ref_args, run_reference

pytestmark = pytest.mark.gpu

N_PACKETS = 1200
LSDR_E_ARG, LSDR_E_UNSUPPORTED = -2, -4
SINGLE = ("step 0 deg", "step 90 deg", "step 180 deg", "step 270 deg")


def _sent_list(rate, n_packets):
    from leansdr_amd import synth_dvbs
    return [bytes(p) for p in synth_dvbs.ts_packets(n_packets, start=1000 * rate)]


class _Batch:
    """The eight captures of tests 1 to 3 on the device, one object, and one decode per `relock` asked for, kept."""

    def __init__(self, capi, ctx):
        import bench_c1
        self.capi, self.ctx = capi, ctx
        self.variants = rc.relock_batch(0, N_PACKETS)
        self.names = [v[0] for v in self.variants]
        self.n = len(self.variants[0][1]) // 2
        self.bufs = [ctx.upload(v) for _, v in self.variants]
        self.cb = capi.CaptureBatch(ctx, len(self.variants), self.n, bench_c1.OMEGA, anf=0, relock=3)
        self.kept = {}

    def run(self, relock):
        if relock not in self.kept:
            self.cb.set_relock(relock)
            res, ts = self.cb.decode([b.ptr for b in self.bufs], self.n)
            chains = rc.assert_exact(self.capi, self.ctx, self.cb, res, ts, self.names, self.cb.unlocked_window, relock)
            stats = [self.cb.relock_stats(i) for i in range(len(self.names))]
            self.kept[relock] = (res, ts, chains, stats)
        return self.kept[relock]

    def close(self):
        self.cb.close()
        for b in self.bufs:
            b.free()


@pytest.fixture(scope="module")
def batch(capi, ctx):
    b = _Batch(capi, ctx)
    yield b
    b.close()


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
def test_relock_3_is_the_windowed_chain_bit_for_bit(batch):
    res, ts, chains, stats = batch.run(3)                    # (assert_exact has compared bytes, counts, TS and the stats record)
    for name, r, st, rs in zip(batch.names, res, chains, stats):
        print(f"{name}: {r['ts_packets']} packets, locked {r['locked']}, next_sync {r['next_sync_calls']}, {rs}")
        assert st["locks"] <= 4, f"{name}: invalid input, the chain locks {st['locks']} times"
        assert rs["exhausted"] == 0, (name, rs)
    by = dict(zip(batch.names, stats))
    assert by["noise only"]["locks"] == 0 and by["noise only"]["passes"] == 0 and by["clean"]["passes"] == 1, by
    assert any(s["drops"] and s["passes"] >= 2 for s in stats), "no capture lost its lock inside a whole-chip stretch: the rewind did not run"


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
def test_relock_1_is_its_chain_and_says_when_it_is_exhausted(batch):
    res, ts, chains, stats = batch.run(1)
    for name, st, rs in zip(batch.names, chains, stats):
        print(f"{name}: chain {dict((k, st[k]) for k in rc.STATS_FIELDS)}")
        assert rs["exhausted"] == st["exhausted"], (name, rs, st)


def test_relock_0_and_an_object_never_asked_are_todays_tail(capi, ctx, batch):
    import bench_c1
    res0, ts0, _, stats0 = batch.run(0)
    fresh = capi.CaptureBatch(ctx, len(batch.names), batch.n, bench_c1.OMEGA, anf=0)
    try:
        res, ts = fresh.decode([b.ptr for b in batch.bufs], batch.n)
        assert res == res0 and ts == ts0
        for i, name in enumerate(batch.names):
            r = res[i]
            words = capi.lib.lsdr_capture_batch_words_dev(fresh.h, i)
            wb, wm, wt, st = _chain_reference(capi, ctx, words, r["symbols"], r["symbols"] // 4 + 65536, fresh.unlocked_window)
            assert fresh.stage_bytes(i, "deconv", r["bytes_deconv"]).tobytes() == wb.tobytes() and r["bytes_deconv"] == len(wb), name
            assert fresh.stage_bytes(i, "mpeg", r["bytes_mpeg"]).tobytes() == wm.tobytes() and r["bytes_mpeg"] == len(wm), name
            assert ts[i] == wt.tobytes() and r["next_sync_calls"] == st["next_sync"] and r["locked"] == st["locked"], (name, r, st)
            assert fresh.relock_stats(i) == stats0[i] == dict(locks=0, drops=0, passes=0, exhausted=0, first_drop_byte=rc.NEVER,
                                                              last_lock_byte=rc.NEVER, next_sync_behind_first_lock=0), name
    finally:
        fresh.close()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
def test_a_step_behind_a_burst_is_recovered(batch):
    res0, ts0, _, _ = batch.run(0)
    res3, ts3, chains3, _ = batch.run(3)
    sent = _sent_list(0, N_PACKETS)
    gained = []
    for i, name in enumerate(batch.names):
        if name not in SINGLE:
            continue
        print(f"{name}: relock 0 {res0[i]['ts_packets']} packets locked {res0[i]['locked']}, relock 3 {res3[i]['ts_packets']} locked {res3[i]['locked']}")
        rc.assert_transmitted(packets(ts3[i]), sent, chains3[i]["locks"], name)
        if res3[i]["locked"] == 1 and res0[i]["locked"] == 0 and res3[i]["ts_packets"] > res0[i]["ts_packets"]:
            gained.append(name)
    assert gained, "no single step ends locked with more packets under relock = 3"


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
def test_a_capture_alone_elsewhere_and_on_a_used_object(capi, ctx, batch):
    import bench_c1
    by = dict(batch.variants)
    n = batch.n
    a, b = by["step 180 deg"], by["step 0 deg"]
    nb, tune_b = (4 * n // 5) & ~1, 2e-5
    bufs = {k: ctx.upload(v) for k, v in (("a", a), ("b", b), ("two", by["two steps"]), ("noise", by["noise only"]))}
    used = capi.CaptureBatch(ctx, 3, n, bench_c1.OMEGA, anf=0, relock=1)
    alone = capi.CaptureBatch(ctx, 1, n, bench_c1.OMEGA, anf=0, relock=3)
    try:
        used.decode_each([bufs["two"].ptr, bufs["noise"].ptr, bufs["a"].ptr], [n, n // 3, n], [0.0, 1e-4, 0.0])      # another batch, relock 1
        used.set_relock(3)
        res, ts = used.decode_each([bufs["b"].ptr, None, bufs["a"].ptr], [nb, 0, n], [tune_b, 0.0, 0.0])
        stats = [used.relock_stats(i) for i in range(3)]
        assert res[1]["ts_packets"] == 0 and res[1]["symbols"] == 0 and ts[1] == b"" and stats[1]["locks"] == 0, (res[1], stats[1])
        for key, length, tune, at in (("a", n, 0.0, 2), ("b", nb, tune_b, 0)):
            r1, t1 = alone.decode_each([bufs[key].ptr], [length], [tune])
            assert r1[0] == res[at] and t1[0] == ts[at] and alone.relock_stats(0) == stats[at], (key, r1[0], res[at], stats[at])
        assert stats[2]["locks"] >= 2 and res[2]["ts_packets"] > 0, (res[2], stats[2])
        # … and it is the capture of the batch of eight
        res3, ts3, _, stats3 = batch.run(3)
        i = batch.names.index("step 180 deg")
        assert res[2] == res3[i] and ts[2] == ts3[i] and stats[2] == stats3[i]
    finally:
        used.close(); alone.close()
        for d in bufs.values():
            d.free()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (3, 5))
def test_punctured_rates_recover_like_the_reference(capi, ctx, rate):
    import bench_c1
    n_packets = 2500
    iq = rc.single_step(rate_capture(rate, n_packets)[0], 180)
    n = len(iq) // 2
    ref = packets(run_reference(ref_args(rate, "--anf", "0"), iq))
    sent = _sent_list(rate, n_packets)
    where = {p: i for i, p in enumerate(sent)}
    # condition on the input: the reference ends locked — its last packet was transmitted in the capture's last tenth
    assert ref and where.get(ref[-1], -1) >= 9 * n_packets // 10, f"invalid input: the reference returns {len(ref)} packets and ends at {where.get(ref[-1]) if ref else None}"
    buf = ctx.upload(iq)
    cb = capi.CaptureBatch(ctx, 1, n, bench_c1.OMEGA, fec=rate, anf=0, relock=3)
    try:
        res, ts = cb.decode([buf.ptr], n)
        st = rc.assert_exact(capi, ctx, cb, res, ts, [f"rate {rate}"], cb.unlocked_window, 3, rate)[0]
        pk = packets(ts[0])
        print(f"rate {rate}: {len(pk)} packets, reference {len(ref)}, chain {dict((k, st[k]) for k in rc.STATS_FIELDS)}, next_sync {st['next_sync']}")
        assert len(pk) >= 200, len(pk)
        tail = pk[-200:]
        # the last 200 packets, less at most 16 at their end, are a contiguous run of the reference's
        best = 0
        for j in (j for j, p in enumerate(ref) if p == tail[0]):
            m = 0
            while m < 200 and j + m < len(ref) and ref[j + m] == tail[m]:
                m += 1
            best = max(best, m)
        assert best >= 200 - 16, f"rate {rate}: {best} of the last 200 packets are a run of the reference's"
    finally:
        cb.close(); buf.free()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
def test_cs16_and_a_2048_byte_window(capi, ctx, batch):
    import bench_c1
    res3, ts3, _, stats3 = batch.run(3)
    by = dict(batch.variants)
    names = ["step 180 deg", "two steps"]
    n = batch.n
    s16 = [((by[k].astype(np.int32) - 128) * 256).astype(np.int16) for k in names]
    bufs16 = [ctx.upload(v) for v in s16]
    cb16 = capi.CaptureBatch(ctx, 2, n, bench_c1.OMEGA, anf=0, in_format=capi.IN_CS16, in_scale=2.0 ** -8, relock=3)
    cbw = capi.CaptureBatch(ctx, 2, n, bench_c1.OMEGA, anf=0, unlocked_window=2048, relock=3)
    try:
        res, ts = cb16.decode([b.ptr for b in bufs16], n)
        for k, name in enumerate(names):
            i = batch.names.index(name)
            assert ts[k] == ts3[i] and res[k]["ts_packets"] == res3[i]["ts_packets"] and cb16.relock_stats(k) == stats3[i], name
        resw, tsw = cbw.decode([batch.bufs[batch.names.index(k)].ptr for k in names], n)
        chains = rc.assert_exact(capi, ctx, cbw, resw, tsw, names, 2048, 3)
        print([(r["ts_packets"], dict((k, st[k]) for k in rc.STATS_FIELDS)) for r, st in zip(resw, chains)])
    finally:
        cb16.close(); cbw.close()
        for b in bufs16:
            b.free()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(capi, ctx, batch):
    import bench_c1
    lib = capi.lib
    st = capi.CaptureRelockStats()
    err = lambda: lib.lsdr_last_error().decode()
    vit = capi.CaptureBatch(ctx, 1, 65536, bench_c1.OMEGA, anf=0, viterbi=True)
    cb = capi.CaptureBatch(ctx, 1, batch.n, bench_c1.OMEGA, anf=0)
    try:
        assert lib.lsdr_capture_relock_set(vit.h, 1) == LSDR_E_UNSUPPORTED and "Viterbi" in err()
        assert lib.lsdr_capture_relock_get(vit.h, 0, C.byref(st)) == LSDR_E_UNSUPPORTED and "Viterbi" in err()
        with pytest.raises(capi.LsdrError):
            capi.CaptureBatch(ctx, 1, 65536, bench_c1.OMEGA, anf=0, viterbi=True, relock=2)
        assert lib.lsdr_capture_relock_set(cb.h, 17) == LSDR_E_ARG and "17" in err()
        assert lib.lsdr_capture_relock_set(cb.h, 16) == 0
        assert lib.lsdr_capture_relock_get(cb.h, 0, C.byref(st)) == LSDR_E_ARG and "wait" in err()      # no batch yet
        cb.run_async([batch.bufs[0].ptr], batch.n)
        assert lib.lsdr_capture_relock_set(cb.h, 2) == LSDR_E_ARG and "in flight" in err()
        assert lib.lsdr_capture_relock_get(cb.h, 0, C.byref(st)) == LSDR_E_ARG and "wait" in err()
        cb.wait()
        assert lib.lsdr_capture_relock_get(cb.h, 1, C.byref(st)) == LSDR_E_ARG and lib.lsdr_capture_relock_get(cb.h, -1, C.byref(st)) == LSDR_E_ARG
        assert lib.lsdr_capture_relock_get(cb.h, 0, C.byref(st)) == 0 and st.locks == 1 and st.exhausted == 0
        assert lib.lsdr_capture_relock_set(cb.h, 2) == 0
    finally:
        vit.close(); cb.close()
