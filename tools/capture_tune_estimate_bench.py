#!/usr/bin/env python3
"""tools/capture_tune_estimate_bench.py [--captures 32] [--msamples 8] [--repeats 7] [--out FILE]

What estimating every capture's carrier offset (lsdr_tune_est) costs next to decoding it, one GPU, generator captures at the bench
condition (bench_c1.Generator: QPSK 1/2, 1.2 samples per symbol, leanchansim --awgn 17.5), cu8 — the shape of `bench.py --workload c1`.
After one warm-up each, `repeats` times on the host clock (every timed call ends in a wait):

  * the estimator alone, run_async → wait, with 8 and with 64 blocks of 4096 samples per capture;
  * the default-engine capture batch (anf 1, tile_len 4096) with the tunes GIVEN (decode_each: run_each_async → wait → TS fetch) beside
    decode_estimated (the estimator with 8 blocks, one host read of B records, then the same decode_each).

The two ratios — estimator over the batch with tunes given, decode_estimated over decode_each — are recorded, no threshold is set.
The decode kernels are the parent commit's: the batch's own time with tunes given is not measured against it.

Writes one JSON line to --out (default profiles/tune_estimate/bench.json) and to stdout."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tune_estimate", "bench.json"))
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
    result = dict(tool="tools/capture_tune_estimate_bench.py", repeats=args.repeats,
                  workload=f"B = {B} x {args.msamples} Mi samples cu8, QPSK 1/2 at 1.2 samples per symbol, generator captures (Es/N0 as leanchansim --awgn 17.5); "
                           "capture batch: default engine, anf 1, tile_len 4096")
    est_s = {}
    for blocks in (8, 64):
        est = capi.TuneEstimator(ctx, B, blocks=blocks)
        first = est.estimate(ptrs, lengths)                                     # warm-up
        ts = timed(lambda: est.estimate(ptrs, lengths), args.repeats)
        est.close()
        est_s[blocks] = statistics.median(ts)
        result[f"estimator_{blocks}_blocks"] = dict(seconds=spread(ts), max_abs_tune=max(abs(e["tune"]) for e in first),
                                                    min_quality=round(min(e["quality"] for e in first), 1), blocks=[e["blocks"] for e in first][:2])
    cb = capi.CaptureBatch(ctx, B, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512)
    res, ts0, estimates = cb.decode_estimated(ptrs, lengths)                    # warm-up of both paths, and what is handed over
    tunes = [e["tune"] if e["quality"] >= capi.TUNE_MIN_QUALITY else 0.0 for e in estimates]
    given = cb.decode_each(ptrs, lengths, tunes)
    result["decode_estimated_returns_decode_each_with_the_estimates"] = bool(given[0] == res and given[1] == ts0)
    result["locked"] = all(r["locked"] == 1 and r["seam_bad"] == 0 for r in res)
    result["ts_packets"] = [r["ts_packets"] for r in res][:4]
    t_given = timed(lambda: cb.decode_each(ptrs, lengths, tunes), args.repeats)
    t_est = timed(lambda: cb.decode_estimated(ptrs, lengths), args.repeats)
    cb.close()
    result["decode_each_tunes_given"] = dict(seconds=spread(t_given))
    result["decode_estimated"] = dict(seconds=spread(t_est))
    g = statistics.median(t_given)
    result["estimator_8_blocks_over_decode_each"] = round(est_s[8] / g, 5)
    result["estimator_64_blocks_over_decode_each"] = round(est_s[64] / g, 5)
    result["decode_estimated_over_decode_each"] = round(statistics.median(t_est) / g, 5)
    for b in bufs:
        b.free()
    ctx.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
