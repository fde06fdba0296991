#!/usr/bin/env python3
"""tools/rate_estimate_bench.py [--captures 32] [--msamples 8] [--repeats 7] [--out FILE]

What estimating every capture's samples per symbol (lsdr_rate_est) costs next to estimating its carrier offset (lsdr_tune_est) and next
to decoding it, one GPU, generator captures at the bench condition (bench_c1.Generator: QPSK 1/2, 1.2 samples per symbol, leanchansim
--awgn 17.5), cu8 — the shape of `bench.py --workload c1`.  After one warm-up each, `repeats` times on the host clock, in one process
(every timed call ends in a wait):

  * the rate estimator alone, run_async → wait, with 64 and with 256 blocks of 4096 samples per capture;
  * the tune estimator alone with 64 blocks: the same bytes read, the same transform;
  * the default-engine capture batch (anf 1, tile_len 4096) constructed with the ESTIMATED omega (the job's one group from
    capi.group_by_omega), tunes given (decode_each: run_each_async → wait → TS fetch).

The ratios are recorded, no threshold is set.  The decode kernels are the parent commit's.

Writes one JSON line to --out (default profiles/rate_estimate/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(ts):
    return dict(median=round(statistics.median(ts), 6), min=round(min(ts), 6), max=round(max(ts), 6), n=len(ts))


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=32)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_estimate", "bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench_c1
    import leansdr_amd.capi as capi
    B, n = args.captures, args.msamples << 20
    ctx = capi.Ctx(0)
    gen = bench_c1.Generator(capi, ctx, n, B)
    bufs = [gen.capture(k, 7000 + k)[0] for k in range(B)]
    gen.close()
    ptrs, lengths = [b.ptr for b in bufs], [n] * B
    result = dict(tool="tools/rate_estimate_bench.py", repeats=args.repeats,
                  workload=f"B = {B} x {args.msamples} Mi samples cu8, QPSK 1/2 at 1.2 samples per symbol, generator captures (Es/N0 as leanchansim --awgn 17.5); "
                           "capture batch: default engine, anf 1, tile_len 4096")
    rate_s, first = {}, None
    for blocks in (64, 256):
        est = capi.RateEstimator(ctx, B, blocks=blocks)
        got = est.estimate(ptrs, lengths)                                       # warm-up
        ts = timed(lambda: est.estimate(ptrs, lengths), args.repeats)
        est.close()
        rate_s[blocks] = statistics.median(ts)
        first = first or got
        result[f"rate_estimator_{blocks}_blocks"] = dict(
            seconds=spread(ts), max_rel_error=float(f"{max(abs(e['omega'] / bench_c1.OMEGA - 1) for e in got):.3e}"),
            min_quality=round(min(e["quality"] for e in got), 1), max_quality=round(max(e["quality"] for e in got), 1),
            ambiguous=sum(e["ambiguous"] for e in got), blocks=[e["blocks"] for e in got][:2])
    te = capi.TuneEstimator(ctx, B, blocks=64)
    tunes = [e["tune"] if e["quality"] >= capi.TUNE_MIN_QUALITY else 0.0 for e in te.estimate(ptrs, lengths)]       # warm-up
    t_tune = timed(lambda: te.estimate(ptrs, lengths), args.repeats)
    te.close()
    result["tune_estimator_64_blocks"] = dict(seconds=spread(t_tune))
    groups, left = capi.group_by_omega(first)
    result["groups"] = [[round(o, 7), len(m)] for o, m in groups]
    result["left_out"] = len(left)
    omega = groups[0][0] if groups else bench_c1.OMEGA
    cb = capi.CaptureBatch(ctx, B, n, omega, anf=1, tile_len=4096, tile_warmup=512)
    res, _ = cb.decode_each(ptrs, lengths, tunes)                               # warm-up
    result["locked"] = all(r["locked"] == 1 and r["seam_bad"] == 0 for r in res)
    result["ts_packets"] = [r["ts_packets"] for r in res][:4]
    t_dec = timed(lambda: cb.decode_each(ptrs, lengths, tunes), args.repeats)
    cb.close()
    result["decode_each_omega_estimated"] = dict(seconds=spread(t_dec))
    g, t = statistics.median(t_dec), statistics.median(t_tune)
    result["rate_64_blocks_over_tune_64_blocks"] = round(rate_s[64] / t, 4)
    result["rate_64_blocks_over_decode_each"] = round(rate_s[64] / g, 5)
    result["rate_256_blocks_over_decode_each"] = round(rate_s[256] / g, 5)
    for b in bufs:
        b.free()
    ctx.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
