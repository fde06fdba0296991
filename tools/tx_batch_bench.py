#!/usr/bin/env python3
"""tools/tx_batch_bench.py [--streams 32] [--packets 4238] [--repeats 5] [--old-repeats 2] [--sweep-packets 1000] [--only-batch] [--out FILE]

What lsdr_tx_batch (leandvbtx | leanchansim for many streams in shared launches) costs and what it is for, one GPU, one process.

(a) Generator timing.  `streams` streams of `packets` leantsgen packets (4238 packets are 8 Mi samples at 6/5), QPSK 1/2, AGC, cu8
    out, amp 75, noise 7.5, a seed per stream.  After one warm-up each, alternating, on the host clock:
      * tx_batch: lsdr_tx_batch_run_async → lsdr_tx_batch_wait, the TS already in device memory;
      * the one-stream blocks: per stream capi.TxChain.run + capi.Wgn.run(add=) + capi.cconv_f32_u8 — every intermediate buffer crosses
        the host, as those wrappers do.  Stream 0's bytes are compared with the batch's.
    Beside them: the kernel launches of a run at B = 1 and B = `streams` (lsdr_tx_batch_stats), and per stage the bytes it reads and
    writes and the time those need at 8 TB/s (a floor for the memory side only; the noise stage draws 2·4/π drand48 pairs, a logf, a
    square root and a division per sample and moves 10 bytes: it is bound by arithmetic).  --only-batch runs nothing but the batch,
    for a kernel trace.
(b) A sensitivity sweep in one batch each: the reference benchmark's series "1.2sps" (22 … 15 dB, leandvb's default graph) and
    "1.2sps-viterbi" (12 … 8.5 dB, --viterbi), 4 seeds per point, `sweep-packets` packets per stream, the signal held at amp 75 with
    AGC and the noise at 37.5 dB − SNR: TxBatch → CaptureBatch.decode_each on the device pointers.  Per point: the packets that came
    back and were sent (per seed), rs_bit_errors per bit of the RS packets; the whole sweep's time (generate + decode).
    And a listing: five streams at the five code rates, what CaptureBatch.estimate_fec says over 16384 symbols.

Nothing is a threshold.  Writes one JSON line to --out (default profiles/tx_batch/bench.json) and to stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
SERIES = {"1.2sps": ([22, 21, 20, 19, 18, 17, 16, 15], False), "1.2sps-viterbi": ([12, 11, 10.5, 10, 9.5, 9, 8.5], True)}
SEEDS = 4


def spread(ts):
    return dict(median=round(statistics.median(ts), 6), min=round(min(ts), 6), max=round(max(ts), 6), n=len(ts))


def stage_bytes(plan, n_packets, ncoeffs=61, interp=6, agc=True, item=2):
    """Bytes one stream's stages read and write (the model, not a measurement)."""
    s, n = plan["symbols"], plan["samples"]
    return {"bytes (randomize + RS)": 188 * n_packets + 204 * n_packets,
            "symbols (interleave gather + coder)": plan["bytes"] + s,
            "samples (FIR from symbol bytes)": s + 8 * n + (4 * n // 128 if agc else 0),
            "agc (EMA walk)": 8 * (n // 128) if agc else 0,
            "noise count + scan": 12 * (n * 4 // (3 * 4096) + 1),
            "emit (gain, scale, + noise, convert)": 8 * n + item * n + (4 * n // 128 if agc else 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--packets", type=int, default=4238)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--old-repeats", type=int, default=2)
    ap.add_argument("--sweep-packets", type=int, default=1000)
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx_batch", "bench.json"))
    a = ap.parse_args()
    import leansdr_amd.capi as capi
    from leansdr_amd import synth_dvbs
    ctx = capi.Ctx(0)
    B, npk = a.streams, a.packets
    out = dict(tool="tx_batch_bench", streams=B, packets=npk)

    # ---- (a)
    ts = [synth_dvbs.ts_packets(npk, start=npk * i) for i in range(B)]
    d_ts = [ctx.upload(t) for t in ts]
    each = [dict(fec=capi.FEC12, amp=75.0, scale=1.0, noise_stddev=7.5, seed=1 + i) for i in range(B)]
    tb = capi.TxBatch(ctx, B, npk, interp=6, decim=5, agc=True, out_format=capi.IN_CU8)
    arr = (capi.TxEach * B)(*[tb.each(n_packets=npk, **e) for e in each])
    ptrs = (capi.vp * B)(*[d.ptr for d in d_ts])
    res = (capi.TxResult * B)()

    def batch():
        capi.check(capi.lib.lsdr_tx_batch_run_async(tb.h, ptrs, arr))
        capi.check(capi.lib.lsdr_tx_batch_wait(tb.h, res))

    def old(i):
        e = each[i]
        tx = capi.TxChain(ctx, interp=6, decim=5, amp=e["amp"], agc=True, rate=e["fec"])
        y = tx.run(ts[i])
        tx.close()
        w = capi.Wgn(ctx, e["seed"])
        z = w.run(len(y), e["noise_stddev"], add=y)                        # scale 1
        w.close()
        return capi.cconv_f32_u8(ctx, z)

    batch()                                                               # warm-up
    plan = tb.plan(each[0], n_packets=npk)
    out["samples_per_stream"] = plan["samples"]
    out["launches"] = {str(B): tb.stats()["launches_last_run"]}
    out["noise_rounds"] = sorted({int(r.noise_rounds) for r in res})
    t_batch, t_old = [], []
    if a.only_batch:
        for _ in range(a.repeats):
            t0 = time.perf_counter(); batch(); t_batch.append(time.perf_counter() - t0)
    else:
        tb._last = [r.as_dict() for r in res]
        first = tb.download(0)
        ref0 = old(0)                                                     # warm-up of the one-stream blocks, and the check
        out["stream0_bits_equal"] = bool(first.shape == ref0.shape and first.tobytes() == ref0.tobytes())
        for k in range(max(a.repeats, a.old_repeats)):
            if k < a.repeats:
                t0 = time.perf_counter(); batch(); t_batch.append(time.perf_counter() - t0)
            if k < a.old_repeats:
                t0 = time.perf_counter()
                for i in range(B):
                    old(i)
                t_old.append(time.perf_counter() - t0)
        one = capi.TxBatch(ctx, 1, npk, interp=6, decim=5, agc=True, out_format=capi.IN_CU8)
        one.run([(d_ts[0].ptr, npk)], [each[0]])
        out["launches"]["1"] = one.stats()["launches_last_run"]
        one.close()
    out["tx_batch_s"] = spread(t_batch)
    out["tx_batch_msamples_per_s"] = round(B * plan["samples"] / statistics.median(t_batch) / 1e6, 1)
    if t_old:
        out["one_stream_blocks_s"] = spread(t_old)
        out["ratio_median"] = round(statistics.median(t_old) / statistics.median(t_batch), 1)
    sb = stage_bytes(plan, npk)
    out["stage_bytes_all_streams"] = {k: v * B for k, v in sb.items()}
    out["stage_us_at_8TBps"] = {k: round(v * B / HBM_BYTES_PER_S * 1e6, 2) for k, v in sb.items()}
    out["all_stages_us_at_8TBps"] = round(sum(sb.values()) * B / HBM_BYTES_PER_S * 1e6, 2)
    tb.close()
    for d in d_ts:
        d.free()

    # ---- (b)
    if not a.only_batch:
        sp = a.sweep_packets
        sweep = {}
        t_sweep = 0.0
        for name, (snrs, viterbi) in SERIES.items():
            n = len(snrs) * SEEDS
            sts = [synth_dvbs.ts_packets(sp, start=7 * k) for k in range(n)]
            d = [ctx.upload(t) for t in sts]
            ea = [dict(fec=capi.FEC12, amp=75.0, scale=1.0, noise_stddev=capi.db_to_amplitude(37.5 - snr), seed=1000 + s)
                  for snr in snrs for s in range(SEEDS)]
            tx = capi.TxBatch(ctx, n, sp, interp=6, decim=5, agc=True, out_format=capi.IN_CU8)
            tin = [(x.ptr, sp) for x in d]
            r = tx.run(tin, ea)                                           # warm-up (allocations, first launches)
            cb = capi.CaptureBatch(ctx, n, max(tx.lengths()), 1.2, fec=capi.FEC12, viterbi=True if viterbi else None)
            cb.decode_each(tx.ptrs(), tx.lengths())
            t0 = time.perf_counter()
            r = tx.run(tin, ea)
            cres, cts = cb.decode_each(tx.ptrs(), tx.lengths())
            dt = time.perf_counter() - t0
            t_sweep += dt
            points = []
            for p, snr in enumerate(snrs):
                seeds = []
                for s in range(SEEDS):
                    k = p * SEEDS + s
                    sent = {bytes(t) for t in sts[k]}
                    pk = np.frombuffer(cts[k], np.uint8).reshape(-1, 188)
                    good = sum(bytes(t) in sent for t in pk)
                    rsb = cres[k]["rs_packets"] * 204 * 8
                    seeds.append(dict(back=len(pk), sent_among_them=good, rs_bit_errors_per_bit=round(cres[k]["rs_bit_errors"] / rsb, 7) if rsb else None))
                points.append(dict(snr_db=snr, noise_stddev=round(ea[p * SEEDS]["noise_stddev"], 4), seeds=seeds))
            sweep[name] = dict(streams=n, packets=sp, samples_per_stream=r[0]["samples"], seconds=round(dt, 4), points=points)
            tx.close(); cb.close()
            for x in d:
                x.free()
        out["sweep"] = sweep
        out["sweep_seconds"] = round(t_sweep, 4)
        # the code-rate listing
        rates = [capi.FEC12, capi.FEC23, capi.FEC34, capi.FEC56, capi.FEC78]
        sts = [synth_dvbs.ts_packets(sp, start=11 * k) for k in range(5)]
        tx = capi.TxBatch(ctx, 5, sp, interp=6, decim=5, agc=True, out_format=capi.IN_CU8)
        tx.run(sts, [dict(fec=f, amp=75.0, scale=1.0, noise_stddev=capi.db_to_amplitude(37.5 - 20), seed=50 + k) for k, f in enumerate(rates)])
        cb = capi.CaptureBatch(ctx, 5, max(tx.lengths()), 1.2, fec=capi.FEC12)
        cres, _ = cb.decode_each(tx.ptrs(), tx.lengths())
        est = cb.estimate_fec(cres, 16384)
        out["estimate_fec"] = [dict(sent=f, fec=e["fec"], locked=e["locked"], ambiguous=e["ambiguous"], error_rate=round(e["error_rate"], 5),
                                    runner_up=round(e["runner_up"], 5)) for f, e in zip(rates, est)]
        tx.close(); cb.close()
    ctx.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
