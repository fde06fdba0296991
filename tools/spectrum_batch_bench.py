#!/usr/bin/env python3
"""tools/spectrum_batch_bench.py [--captures 32] [--msamples 8] [--repeats 5] [--baseline-captures 2] [--out FILE]

What lsdr_spectrum_batch costs, one GPU: B cu8 captures of `msamples` Mi samples (a synthetic DVB-S capture at 4 samples per symbol,
repeated to length, every capture in a buffer of its own).  After one warm-up each, `repeats` times; `seconds` is the host clock around
run_async → wait, `kernel_ms` the stream's events around what run_async queues.

  (i)  leandvb's own setting: cnr_fft, nfft 4096, a value every 2 Mi samples (four rows per capture), bandwidth 1/4;
  (ii) the dense case (every block a row) with rows emitted: nfft 4096 (with the CNR) and nfft 1024, each with four radix-2 stages per
       pass (16 points per thread in registers) and with one (k_cfft's form: a barrier and an LDS round trip per stage).

Each figure stands beside the same job through the EXISTING single-stream objects (capi.CnrFft, lsdr_spectrum_run) on a cf32 copy of a
capture, one capture after the other: measured on `baseline-captures` captures and scaled to B (they are the parent's code and not under
test).  The dense case also stands beside the bytes it must move (captures in, kept rows out) over 8 TB/s.  No threshold is set: the
figures are recorded.

Writes one JSON line to --out (default profiles/spectrum_batch/bench.json) and to stdout."""
import argparse
import ctypes as C
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


def batch_case(capi, ctx, B, n, ptrs, repeats, keep_bytes, **kw):
    """One SpectrumBatch configuration: dict of its figures."""
    sb = capi.SpectrumBatch(ctx, B, n, **kw)
    lengths, centers = [n] * B, [0.0] * B
    sb.run_async(ptrs, lengths, centers)                                            # warm-up
    res = sb.wait()
    host, kernel = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        sb.run_async(ptrs, lengths, centers)
        sb.wait()
        host.append(time.perf_counter() - t0)
    for _ in range(repeats):
        ctx.timer_start()
        sb.run_async(ptrs, lengths, centers)
        kernel.append(ctx.timer_stop_ms())
        sb.wait()
    rows = sum(r["rows"] for r in res)
    out = dict(seconds=spread(host), kernel_ms=spread(kernel, 4), rows=rows, slab_rows=sb.slab_rows, transforms_per_s=round(rows / (statistics.median(kernel) * 1e-3), 1))
    if sb.bandwidth > 0:
        out["cnr_first_capture"] = [round(float(v), 3) for v in sb.cnr_db(0)[:4]]
    if keep_bytes:
        nbytes = B * n * 2 + rows * sb.nfft * 4
        k = statistics.median(kernel) * 1e-3
        out.update(bytes=nbytes, bytes_over_8TBps_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 4), achieved_TBps=round(nbytes / k / 1e12, 3),
                   capture_bytes_over_8TBps_ms=round(B * n * 2 / HBM_BYTES_PER_S * 1e3, 4), Gsamples_per_s=round(B * n / k / 1e9, 3))
    sb.close()
    return out


def single_cnr(capi, ctx, ptr, n, nfft, dec, count):
    """capi.CnrFft on the cf32 copy, `count` captures one after the other (a new object each): seconds per capture."""
    ts = []
    for _ in range(count + 1):                                                      # the first is the warm-up
        c = capi.CnrFft(ctx, 0.25, nfft, dec)
        t0 = time.perf_counter()
        out, cons = c.run_dev(ptr, n, 0.0, 1.0)
        ts.append(time.perf_counter() - t0)
        c.close()
    return dict(seconds_per_capture=spread(ts[1:]), values=len(out))


def single_spectrum(capi, ctx, ptr, n, dec, count):
    """lsdr_spectrum_run on the cf32 copy with room for every row: seconds per capture."""
    rows = np.empty((n // 1024 + 1, 1024), np.float32)
    ts = []
    for _ in range(count + 1):
        sp = capi.Spectrum(ctx, dec, 0.5)
        cons, prod = C.c_size_t(), C.c_size_t()
        t0 = time.perf_counter()
        capi.check(capi.lib.lsdr_spectrum_run(sp.h, ptr, n, rows.ctypes.data_as(C.c_void_p), len(rows), C.byref(cons), C.byref(prod)))
        ts.append(time.perf_counter() - t0)
        sp.close()
    return dict(seconds_per_capture=spread(ts[1:]), rows=prod.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=32)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-captures", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_batch", "bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import leansdr_amd.capi as capi
    from leansdr_amd import synth_dvbs
    B, n, sps = args.captures, args.msamples << 20, 4
    piece = 1 << 20
    iq, _ = synth_dvbs.capture_u8(n_packets=piece // (1632 * sps) + 2, sps_num=sps, sps_den=1, seed=11, noise_std=7.5)
    host = np.tile(np.ascontiguousarray(iq[: 2 * piece]), n // piece)
    ctx = capi.Ctx(0)
    bufs = [ctx.upload(host) for _ in range(B)]
    ptrs = [b.ptr for b in bufs]
    f32 = ctx.upload((host.astype(np.float32) - 128).view(np.complex64))
    result = dict(tool="tools/spectrum_batch_bench.py", repeats=args.repeats, library=os.path.basename(capi.LIB_PATH),
                  workload=f"B = {B} x {args.msamples} Mi samples cu8, synthetic DVB-S QPSK 1/2 at {sps} samples per symbol, noise 7.5")
    K = args.baseline_captures

    # ---- (i) leandvb's own setting
    dec = 2 << 20
    result["leandvb_cnr"] = batch_case(capi, ctx, B, n, ptrs, args.repeats, False, nfft=4096, decimation=dec, bandwidth=0.25)
    one = single_cnr(capi, ctx, f32.ptr, n, 4096, dec, K)
    one["seconds_for_B"] = round(one["seconds_per_capture"]["median"] * B, 6)
    result["leandvb_cnr_single_stream"] = one
    result["leandvb_cnr_single_stream_over_batch"] = round(one["seconds_for_B"] / result["leandvb_cnr"]["seconds"]["median"], 2)

    # ---- (ii) dense, rows emitted
    for nfft in (4096, 1024):
        bw = 0.25 if nfft == 4096 else 0.0
        for stages in (4, 1):
            name = f"dense_{nfft}_stages{stages}"
            result[name] = batch_case(capi, ctx, B, n, ptrs, args.repeats, True, nfft=nfft, decimation=nfft, bandwidth=bw, rows=True,
                                      kavg=0.1 if nfft == 4096 else 0.5, stages_per_pass=stages)
        result[f"dense_{nfft}_stages1_over_stages4"] = round(result[f"dense_{nfft}_stages1"]["kernel_ms"]["median"] /
                                                             result[f"dense_{nfft}_stages4"]["kernel_ms"]["median"], 3)
    one = single_cnr(capi, ctx, f32.ptr, n, 4096, 4096, K)
    one["seconds_for_B"] = round(one["seconds_per_capture"]["median"] * B, 4)
    result["dense_4096_single_stream"] = one
    result["dense_4096_single_stream_over_batch"] = round(one["seconds_for_B"] / result["dense_4096_stages4"]["seconds"]["median"], 1)
    one = single_spectrum(capi, ctx, f32.ptr, n, 1024, K)
    one["seconds_for_B"] = round(one["seconds_per_capture"]["median"] * B, 4)
    result["dense_1024_single_stream"] = one
    result["dense_1024_single_stream_over_batch"] = round(one["seconds_for_B"] / result["dense_1024_stages4"]["seconds"]["median"], 1)

    for b in bufs + [f32]:
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
