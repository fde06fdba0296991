#!/usr/bin/env python3
"""tools/resample_batch_bench.py [--captures 32] [--msamples 8] [--repeats 7] [--out FILE]

What lsdr_resample_batch costs, one GPU.  After one warm-up each, `repeats` times; `seconds` is the host clock around run → wait,
`kernel_ms` the stream's events around the queued run (the upload of B records and the one launch).

  * resampler alone: B cu8 captures of `msamples` Mi samples at omega 12 (leandvb's filter for it: D = 3, N = 33), synthetic DVB-S
    captures at four carrier offsets, every capture in a buffer of its own, tunes given;
  * ResampledDecoder.decode on the same captures (default engine, anf 0), whole and split into its four steps: the raw estimate, the
    resampler, the fine estimate on the decimated streams, decode_each;
  * one cf32 geometry with D = 30, N = 313 (omega 120): 8 captures of `msamples` Mi samples of noise.

Each resampler figure stands beside two yardsticks: the bytes the kernel must move (the captures in, the cf32 streams out) over 8 TB/s,
and the single-stream FirFilter(arith=FIR_EXACT) of the same geometry and format on ONE capture (per input sample; it has no rotator and
serves one stream per launch — it is the parent's kernel and is not under test).  No threshold is set: the figures are recorded.

Writes one JSON line to --out (default profiles/resample_batch/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12


def spread(ts, digits=6):
    return dict(median=round(statistics.median(ts), digits), min=round(min(ts), digits), max=round(max(ts), digits), n=len(ts))


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def resampler_alone(capi, ctx, rs, ptrs, lengths, tunes, outs, cap_out, item_bytes, repeats):
    """The resampler's figures and its two yardsticks' inputs: dict."""
    res = rs.run(ptrs, lengths, tunes, outs, cap_out)                               # warm-up
    host = timed(lambda: rs.run(ptrs, lengths, tunes, outs, cap_out), repeats)
    kernel = []
    for _ in range(repeats):
        ctx.timer_start()
        rs.run_async(ptrs, lengths, tunes, outs, cap_out)
        kernel.append(ctx.timer_stop_ms())
        rs.wait()
    n_in, n_out = sum(lengths), sum(r["produced"] for r in res)
    nbytes = n_in * item_bytes + n_out * 8
    k = statistics.median(kernel) * 1e-3
    return dict(seconds=spread(host), kernel_ms=spread(kernel, 4), tile=rs.tile, samples_in=n_in, items_out=n_out, bytes=nbytes,
                bytes_over_8TBps_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 4), achieved_TBps=round(nbytes / k / 1e12, 3),
                ns_per_input_sample=round(k / n_in * 1e9, 5), Gsamples_per_s=round(n_in / k / 1e9, 3))


def single_stream(capi, ctx, coeffs, decim, in_format, ptr, n, out_ptr, cap_out, repeats):
    """The parent's FirFilter(FIR_EXACT) on one capture: dict."""
    fir = capi.FirFilter(ctx, coeffs, decim, in_format=in_format, arith=capi.FIR_EXACT)
    fir.run_dev(ptr, n, out_ptr, cap_out)                                           # warm-up
    kernel = []
    for _ in range(repeats):
        ctx.timer_start()
        cons, prod = fir.run_dev(ptr, n, out_ptr, cap_out)
        kernel.append(ctx.timer_stop_ms())
    fir.close()
    k = statistics.median(kernel) * 1e-3
    return dict(kernel_ms=spread(kernel, 4), produced=prod, ns_per_input_sample=round(k / n * 1e9, 5), Gsamples_per_s=round(n / k / 1e9, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=32)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_batch", "bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import leansdr_amd.capi as capi
    from leansdr_amd import synth_dvbs
    B, n, sps = args.captures, args.msamples << 20, 12
    offsets = [0.0, 0.01, -0.03, 0.1]
    iq, _ = synth_dvbs.capture_u8(n_packets=n // (1632 * sps) + 2, sps_num=sps, sps_den=1, seed=11, noise_std=7.5)
    iq = np.ascontiguousarray(iq[: 2 * n])
    a = iq.reshape(-1, 2).astype(np.float64) - 128
    z = a[:, 0] + 1j * a[:, 1]
    k = np.arange(n)
    hosts = []
    for f in offsets:
        s = z * np.exp(2j * np.pi * f * k) if f else z
        hosts.append(np.clip(np.rint(np.stack([s.real, s.imag], axis=1) + 128), 0, 255).astype(np.uint8).reshape(-1))
    del a, z, k
    ctx = capi.Ctx(0)
    bufs = [ctx.upload(hosts[i % len(offsets)]) for i in range(B)]
    tunes = [offsets[i % len(offsets)] for i in range(B)]
    ptrs, lengths = [b.ptr for b in bufs], [n] * B
    result = dict(tool="tools/resample_batch_bench.py", repeats=args.repeats,
                  workload=f"B = {B} x {args.msamples} Mi samples cu8, synthetic DVB-S QPSK 1/2 at {sps} samples per symbol, noise 7.5, offsets {offsets}")

    # ---- the resampler alone, omega 12
    dec = capi.ResampledDecoder(ctx, B, n, float(sps), anf=0)
    outs = [b.ptr for b in dec._outs]
    result["geometry_cu8"] = dict(decim=dec.decim, ncoeffs=len(dec.coeffs), omega_out=dec.omega_out)
    result["resampler_cu8"] = resampler_alone(capi, ctx, dec.resampler, ptrs, lengths, tunes, outs, dec.cap_out, 2, args.repeats)
    result["single_stream_fir_exact_cu8"] = single_stream(capi, ctx, dec.coeffs, dec.decim, capi.IN_CU8, ptrs[0], n, outs[0], dec.cap_out, args.repeats)
    result["resampler_cu8_over_single_stream_per_sample"] = round(result["resampler_cu8"]["ns_per_input_sample"] /
                                                                  result["single_stream_fir_exact_cu8"]["ns_per_input_sample"], 4)

    # ---- ResampledDecoder.decode, whole and in its four steps
    res, ts, info = dec.decode(ptrs, lengths)                                       # warm-up; what the steps below are handed
    result["decode"] = dict(locked=all(r["locked"] == 1 for r in res), seam_bad=sum(r["seam_bad"] for r in res), ts_packets=[r["ts_packets"] for r in res][:4],
                            raw_tune=[round(i["tune_raw"], 7) for i in info][:4], fine_tune=[round(i["tune"], 8) for i in info][:4],
                            min_quality_raw=round(min(i["raw"]["quality"] for i in info), 1), min_quality_fine=round(min(i["fine"]["quality"] for i in info), 1))
    t_raw = [i["tune_raw"] for i in info]
    t_dec = [i["tune"] for i in info]
    produced = [i["produced"] for i in info]
    steps = dict(raw_estimate=lambda: dec.est_raw.estimate(ptrs, lengths),
                 resample=lambda: dec.resampler.run(ptrs, lengths, t_raw, outs, dec.cap_out),
                 fine_estimate=lambda: dec.est_fine.estimate(outs, produced),
                 decode_each=lambda: dec.batch.decode_each(outs, produced, t_dec),
                 whole=lambda: dec.decode(ptrs, lengths))
    result["decode_steps_seconds"] = {name: spread(timed(fn, args.repeats)) for name, fn in steps.items()}
    whole = result["decode_steps_seconds"]["whole"]["median"]
    result["decode_Msamples_per_s"] = round(B * n / whole / 1e6, 1)
    dec.close()
    for b in bufs:
        b.free()

    # ---- cf32, D = 30, N = 313
    B2 = 8
    decim, coeffs = capi.resample_design(120.0)
    rng = np.random.default_rng(3)
    noise = (rng.standard_normal(2 * n) * 50).astype(np.float32)
    bufs = [ctx.upload(np.roll(noise, 2 * 1000 * i)) for i in range(B2)]
    cap_out = (n - len(coeffs)) // decim
    outb = [ctx.alloc(cap_out * 8) for _ in range(B2)]
    rs = capi.ResampleBatch(ctx, B2, n, coeffs, decim, in_format=capi.IN_CF32)
    ptrs, outs = [b.ptr for b in bufs], [b.ptr for b in outb]
    result["geometry_cf32"] = dict(decim=decim, ncoeffs=len(coeffs), captures=B2)
    result["resampler_cf32"] = resampler_alone(capi, ctx, rs, ptrs, [n] * B2, [0.001 * (i - 3) for i in range(B2)], outs, cap_out, 8, args.repeats)
    result["single_stream_fir_exact_cf32"] = single_stream(capi, ctx, coeffs, decim, capi.IN_CF32, ptrs[0], n, outs[0], cap_out, args.repeats)
    result["resampler_cf32_over_single_stream_per_sample"] = round(result["resampler_cf32"]["ns_per_input_sample"] /
                                                                   result["single_stream_fir_exact_cf32"]["ns_per_input_sample"], 4)
    rs.close()
    for b in bufs + outb:
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
