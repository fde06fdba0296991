#!/usr/bin/env python3
"""tools/fec_estimate_bench.py [--streams 32] [--msamples 8] [--repeats 7] [--out FILE]

What estimating every stream's code rate (lsdr_fec_est) costs, one GPU.  After one warm-up each, `repeats` times on the host clock, in one
process (every timed call ends in a wait):

  * the estimator alone, run_async → wait, on `streams` streams of 16 Ki and of 1 Mi uniformly random symbols in each input format
    (max_symbols = the length: every symbol is scored).  Next to each time: the bytes the score kernel reads (the symbols once, plus 48
    symbols of history per tile) divided by 8 TB/s — the kernel is arithmetic (80 parity checks per symbol), not traffic;
  * the same on packed symbols with 1, 2, 4 and 8 runs of 12 refill ends per thread (tiles of 3072 … 24576 symbols; the tuning hook
    LSDR_FEC_EST_GROUPS, read at create): what the shipped tile was chosen from;
  * the two costs the sibling estimators are quoted against, at the bench condition (bench_c1.Generator: QPSK 1/2, 1.2 samples per symbol,
    leanchansim --awgn 17.5, cu8): lsdr_rate_est with 64 blocks, and the default-engine capture batch (anf 1, tile_len 4096) decoding
    `streams` captures of `msamples` Mi samples; and estimate_fec on the decisions that decode left on the device (16384 symbols each).

The ratios are recorded, no threshold is set.  The decode kernels are the parent commit's.

Writes one JSON line to --out (default profiles/fec_estimate/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12


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
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fec_estimate", "bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench_c1
    import leansdr_amd.capi as capi
    B = args.streams
    ctx = capi.Ctx(0)
    result = dict(tool="tools/fec_estimate_bench.py", repeats=args.repeats, streams=B)
    rng = np.random.default_rng(17)
    formats = (("packed", capi.HSYM_PACKED2, 0.25), ("u8", capi.HSYM_U8, 1.0), ("soft", capi.HSYM_SOFT, 4.0))

    def one(fmt, bytes_per_symbol, n, buf):
        stride = int(n * bytes_per_symbol)
        est = capi.FecEstimator(ctx, B, n, fmt)
        tile = est.tile
        ptrs, lengths = [buf.at(i * stride) for i in range(B)], [n] * B
        got = est.estimate(ptrs, lengths)                                       # warm-up
        ts = timed(lambda: est.estimate(ptrs, lengths), args.repeats)
        est.close()
        tiles = -(-n // tile)
        read = B * (n + 48 * tiles) * bytes_per_symbol
        return dict(seconds=spread(ts), tile=tile, read_bytes=int(read), read_over_8TBps_seconds=float(f"{read / HBM_BYTES_PER_S:.3e}"),
                    locked=sum(e["locked"] for e in got), min_error_rate=round(min(e["error_rate"] for e in got), 4))

    for n in (16384, 1 << 20):
        for name, fmt, bps in formats:
            raw = rng.integers(0, 1 << 32, int(B * n * bps) // 4, dtype=np.uint32)     # random bits in every format: random symbols
            buf = ctx.upload(raw)
            result[f"{name}_{n}_symbols"] = one(fmt, bps, n, buf)
            if name == "packed":
                sweep = {}
                for groups in (1, 2, 4, 8):
                    os.environ["LSDR_FEC_EST_GROUPS"] = str(groups)
                    r = one(fmt, bps, n, buf)
                    sweep[str(r["tile"])] = r["seconds"]["median"]
                del os.environ["LSDR_FEC_EST_GROUPS"]
                result[f"packed_{n}_symbols_by_tile"] = sweep
            buf.free()

    n = args.msamples << 20
    gen = bench_c1.Generator(capi, ctx, n, B)
    bufs = [gen.capture(k, 7000 + k)[0] for k in range(B)]
    gen.close()
    ptrs, lengths = [b.ptr for b in bufs], [n] * B
    result["workload"] = (f"B = {B} x {args.msamples} Mi samples cu8, QPSK 1/2 at 1.2 samples per symbol, generator captures (Es/N0 as leanchansim "
                          "--awgn 17.5); capture batch: default engine, anf 1, tile_len 4096")
    re = capi.RateEstimator(ctx, B, blocks=64)
    re.estimate(ptrs, lengths)                                                  # warm-up
    t_rate = timed(lambda: re.estimate(ptrs, lengths), args.repeats)
    re.close()
    result["rate_estimator_64_blocks"] = dict(seconds=spread(t_rate))
    cb = capi.CaptureBatch(ctx, B, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512)
    res, _ = cb.decode(ptrs, n)                                                 # warm-up
    result["ts_packets"] = [r["ts_packets"] for r in res][:4]
    t_dec = timed(lambda: cb.decode(ptrs, n), args.repeats)
    result["decode"] = dict(seconds=spread(t_dec))
    got = cb.estimate_fec(res)                                                  # warm-up
    t_fec = timed(lambda: cb.estimate_fec(res), args.repeats)
    cb.close()
    rates = [sorted(e["score"][i]["errors"] / e["score"][i]["checks"] for e in got) for i in range(5)]
    result["estimate_fec_after_decode"] = dict(
        seconds=spread(t_fec), symbols=got[0]["symbols"], fec=sorted({e["fec"] for e in got}), locked=sum(e["locked"] for e in got),
        ambiguous=sum(e["ambiguous"] for e in got), error_rate=[round(rates[0][0], 4), round(rates[0][-1], 4)],
        lowest_wrong_rate=round(min(r[0] for r in rates[1:]), 4))
    result["estimate_fec_over_decode"] = round(statistics.median(t_fec) / statistics.median(t_dec), 5)
    result["estimate_fec_over_rate_64_blocks"] = round(statistics.median(t_fec) / statistics.median(t_rate), 4)
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
