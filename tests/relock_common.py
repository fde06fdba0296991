"""Shared helpers of the re-acquisition tests (lsdr_capture_relock_set): captures whose carrier comes back on another rotation
behind a burst, and THE LOOP the feature is defined by — deconvol_sync one `window` ahead of mpeg_sync until the (relocks+1)-th lock,
the whole remainder in one call from then on while mpeg_sync is locked — on the oracle's blocks (chain_cpu) and on the GPU's
one-block-per-call C ABI (chain_gpu: batch_common._chain_reference with the cap rule changed, and the counts of the stats record).
relocks = 0 is _chain_reference's own schedule.
"""
import ctypes as C
import functools

import numpy as np
from batch_common import HostTail, noise_only, rate_capture, rotate_u8, with_burst

QUARTER = {0: 0, 90: 1, 180: 2, 270: 3}
NEVER = (1 << 64) - 1


def step_capture(iq, steps):
    """The capture with, for every (start sample, degrees) of `steps` in order: n/40 samples of garbage from `start` on (with_burst, drawn
    from one default_rng(5) burst after burst), then everything behind the middle of that burst — the burst's second half included —
    turned by `degrees` (rotate_u8): a carrier that comes back from the fade on another rotation.  Steps add up."""
    n = len(iq) // 2
    burst = n // 40
    rng = np.random.default_rng(5)
    out = iq.copy()
    for start, deg in steps:
        out = with_burst(out, start, burst, rng)
        mid = start + burst // 2
        out[2 * mid:] = rotate_u8(out[2 * mid:], QUARTER[deg])
    return np.ascontiguousarray(out)


def single_step(iq, deg):
    return step_capture(iq, [(len(iq) // 2 // 2, deg)])                  # (the burst begins at sample n/2)


def two_steps(iq):
    n = len(iq) // 2
    return step_capture(iq, [(n // 3, 180), (2 * n // 3, 270)])


def three_steps(iq):
    n = len(iq) // 2
    return step_capture(iq, [(n // 4, 90), (n // 2, 180), (3 * n // 4, 270)])


def relock_batch(rate=0, n_packets=1200):
    """[(name, IQ)] of the exactness tests: clean; steps of 0, 90, 180 and 270 degrees at n/2; two steps; three steps; noise only."""
    iq = rate_capture(rate, n_packets)[0]
    out = [("clean", iq)]
    out += [(f"step {d} deg", single_step(iq, d)) for d in (0, 90, 180, 270)]
    out += [("two steps", two_steps(iq)), ("three steps", three_steps(iq))]
    out.append(("noise only", noise_only(len(iq) // 2, np.random.default_rng(5))))
    return out


@functools.lru_cache(maxsize=None)
def _oracle():
    import pyoracle
    return pyoracle.Oracle()


def oracle_symbols(iq):
    """The soft symbols of the oracle's serial cstln_receiver (linear sampler, omega 1.2) on a cu8 capture."""
    import pyoracle as po
    a = iq.reshape(-1, 2).astype(np.float32) - np.float32(128)
    x = (a[:, 0] + 1j * a[:, 1]).astype(np.complex64)
    return np.ascontiguousarray(_oracle().rx(po.rx_params(sampler=1, cstln=1, omega=1.2), x)["sym"])


def chain_cpu(oracle, sym, rate, window, relocks, bulk_rule=None):
    """The loop on the oracle's deconvol_sync and mpeg_sync (lo_deconv_run, lo_mpeg_sync_run, lo_deconv_next_sync), then deinterleaver,
    rs_decoder and derandomizer.  bulk_rule(locked, locks) → whether a call has the whole remainder for room (None: the feature's rule).
    Returns dict(ts: [packets], bytes, mpeg, locked, locks, drops, next_sync, exhausted)."""
    L = oracle.lib
    c_sz = C.c_size_t
    sym = np.ascontiguousarray(sym)
    byte_cap = len(sym) // 4 + 65536
    dec, ms = L.lo_deconv_new(rate, 0), L.lo_mpeg_sync_new(0)
    data, mpeg = np.empty(byte_cap + 64, np.uint8), np.empty(byte_cap + 64, np.uint8)
    st, lt = np.empty(byte_cap // 204 + 64, np.int32), np.empty(byte_cap // 204 + 64, np.uint64)
    pos = bw = br = mw = 0
    locks = drops = calls = exhausted = 0
    rule = bulk_rule or (lambda locked, k: locked and k > relocks)
    while True:
        locked = bool(L.lo_mpeg_sync_locked(ms))
        bulk = bool(rule(locked, locks))
        cap = byte_cap - bw if bulk else min(window, byte_cap - bw)
        c = c_sz()
        p = L.lo_deconv_run(dec, sym[pos:].ctypes.data, len(sym) - pos, data[bw:].ctypes.data, cap, C.byref(c))
        if not p:
            break
        pos += c.value; bw += p
        while True:                                                  # mpeg_sync::run() until nothing moves
            was = bool(L.lo_mpeg_sync_locked(ms))
            cc, ns, nl, cns = c_sz(), c_sz(), c_sz(), C.c_int()
            got = L.lo_mpeg_sync_run(ms, data[br:].ctypes.data, bw - br, mpeg[mw:].ctypes.data, byte_cap - mw, C.byref(cc),
                                     st.ctypes.data, len(st), C.byref(ns), lt.ctypes.data, len(lt), C.byref(nl), C.byref(cns))
            now = bool(L.lo_mpeg_sync_locked(ms))
            locks += (not was) and now
            if was and not now:
                drops += 1
                exhausted |= int(bulk)
            if cns.value:
                L.lo_deconv_next_sync(dec)
                calls += 1
            if not got and not cc.value:
                break
            br += cc.value; mw += got
    locked = int(bool(L.lo_mpeg_sync_locked(ms)))
    L.lo_deconv_free(dec); L.lo_mpeg_sync_free(ms)
    pk = oracle.deinterleaver(mpeg[:mw])
    ts = []
    if len(pk):
        msgs, _, _ = oracle.rs_decoder(pk)
        ts = [bytes(p) for p in oracle.derandomizer(msgs)]
    return dict(ts=ts, bytes=data[:bw].copy(), mpeg=mpeg[:mw].copy(), locked=locked, locks=int(locks), drops=drops, next_sync=calls,
                exhausted=exhausted)


def chain_gpu(capi, ctx, words, nsym, byte_cap, window, relocks, rate=0):
    """The loop on capi.Deconv.run_dev_hs2 and HostTail: batch_common._chain_reference, except that a call made while mpeg_sync is locked
    has the whole remainder for room only from the (relocks+1)-th lock on.  Returns (deconvolved bytes, mpeg bytes, TS bytes, stats);
    stats has HostTail.finish's npk, errs, locked, then next_sync, alignment, first_lock_byte and the fields of the stats record: locks,
    drops, exhausted, first_drop_byte, last_lock_byte, next_sync_behind_first_lock."""
    dec, t = capi.Deconv(ctx, rate), HostTail(capi, ctx, byte_cap)
    pos = 0
    s = dict(next_sync=0, alignment=0, locks=0, drops=0, exhausted=0, first_lock_byte=NEVER, first_drop_byte=NEVER, last_lock_byte=NEVER,
             next_sync_behind_first_lock=0)
    while True:
        bulk = t.msync.locked and s["locks"] > relocks
        cap = byte_cap - t.bw if bulk else min(window, byte_cap - t.bw)
        c, p = dec.run_dev_hs2(words, pos, nsym - pos, t.d_bytes.at(t.bw), cap)
        if not p:
            break
        pos += c; t.bw += p
        while True:                                                  # HostTail.sync with the transitions counted
            was = t.msync.locked
            c, p, _, _, cns = t.msync.run_dev(t.d_bytes.at(t.br), t.bw - t.br, t.d_mpeg.at(t.mw), byte_cap - t.mw)
            now = t.msync.locked
            if now and not was:
                s["locks"] += 1
                s["last_lock_byte"] = t.br + c
                if s["first_lock_byte"] == NEVER:
                    s["first_lock_byte"] = t.br + c
            if was and not now:
                s["drops"] += 1
                s["exhausted"] |= int(bulk)
                if s["first_drop_byte"] == NEVER:
                    s["first_drop_byte"] = t.br + c
            if cns:
                dec.next_sync()
                s["next_sync"] += 1
                s["alignment"] = (s["alignment"] + 1) % 4
                s["next_sync_behind_first_lock"] += s["first_lock_byte"] != NEVER
            if not c and not p:
                break
            t.br += c; t.mw += p
    want_bytes, want_mpeg, want_ts, st = t.finish()
    dec.close()
    return want_bytes, want_mpeg, want_ts, dict(st, **s)


STATS_FIELDS = ("locks", "drops", "exhausted", "first_drop_byte", "last_lock_byte", "next_sync_behind_first_lock")


def assert_exact(capi, ctx, cb, res, ts, names, window, relocks, rate=0):
    """Every capture of a waited-for batch against chain_gpu on the object's own packed decisions, bit for bit; returns the chains' stats."""
    out = []
    for i, name in enumerate(names):
        r = res[i]
        words = capi.lib.lsdr_capture_batch_words_dev(cb.h, i)
        byte_cap = r["symbols"] // 4 + 65536            # (the object's own is at least this; a cap rule that binds would differ)
        wb, wm, wt, st = chain_gpu(capi, ctx, words, r["symbols"], byte_cap, window, relocks, rate)
        got_bytes, got_mpeg = cb.stage_bytes(i, "deconv", r["bytes_deconv"]), cb.stage_bytes(i, "mpeg", r["bytes_mpeg"])
        assert r["bytes_deconv"] == len(wb) and got_bytes.tobytes() == wb.tobytes(), (name, r["bytes_deconv"], len(wb))
        assert r["bytes_mpeg"] == len(wm) and got_mpeg.tobytes() == wm.tobytes(), (name, r["bytes_mpeg"], len(wm))
        assert (r["rs_packets"], r["rs_bit_errors"], r["locked"]) == (st["npk"], st["errs"], st["locked"]), (name, r, st)
        assert (r["next_sync_calls"], r["alignment"], r["first_lock_byte"]) == (st["next_sync"], st["alignment"], st["first_lock_byte"]), (name, r, st)
        assert ts[i] == wt.tobytes() and r["ts_packets"] * 188 == len(wt), (name, r["ts_packets"], len(wt) // 188)
        if relocks:
            rs = cb.relock_stats(i)
            assert {k: rs[k] for k in STATS_FIELDS} == {k: st[k] for k in STATS_FIELDS}, (name, rs, st)
        out.append(st)
    return out


DERAND_LAG = 7      # packets: the derandomizer restarts its sequence at an inverted sync byte, one packet in eight (dvb.h:1131-1160)


def assert_transmitted(pk, sent, locks, name):
    """Every TS packet from index bench_c1.SKIP_ACQ on was transmitted — except, behind a RE-acquisition, the packets the derandomizer
    passes before it meets its first inverted sync byte: mpeg_sync locks on any packet of the group of eight, the derandomizer keeps
    every packet whose first byte is 0x47 and de-scrambles it with the sequence position it counted on from the last group, so up to seven
    packets leave with the wrong sequence (the reference's own TS has them; behind the FIRST lock they are what SKIP_ACQ skips).  Such
    runs are at most DERAND_LAG packets long, sit where the transmitted packets' numbers jump, and there are at most locks − 1 of them.
    pk: [packets]; sent: the transmitted packets in order."""
    import bench_c1
    where = {p: i for i, p in enumerate(sent)}
    runs, run, last = [], 0, None
    for i, p in enumerate(pk):
        if i < bench_c1.SKIP_ACQ:
            continue
        j = where.get(p)
        if j is None:
            run += 1
            continue
        if run:
            assert last is None or j > last + run + 1, f"{name}: {run} packets that were never transmitted in front of packet {i}, inside a run of transmitted ones"
            runs.append(run)
            run = 0
        last = j
    if run:
        runs.append(run)
    assert all(r <= DERAND_LAG for r in runs) and len(runs) <= max(locks - 1, 0), f"{name}: runs of packets that were never transmitted: {runs}, {locks} locks"
    return runs
