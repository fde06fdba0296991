#!/usr/bin/env python3
"""tools/capture_batch_formats_bench.py [--captures 16] [--msamples 8] [--repeats 5] [--formats cu8,cs8,cu16,cs16,cf32] [--out FILE]

The capture batch on every sample format (lsdr_capture_any_create), one GPU: B generator captures at the bench condition
(bench_c1.Generator: QPSK 1/2, 1.2 samples per symbol, leanchansim --awgn 17.5) of `msamples` Mi samples, anf 1, tile_len 4096.  The cu8
capture u is the signal; s = u − 128 is given to the other formats as

    cs8 s        cu16 256·s + 32768, in_scale 2^-8        cs16 256·s, in_scale 2^-8        cf32 float(s) / 64, in_scale 64

so every object decodes the same floats and must return the cu8 object's TS (checked before the clock starts).  Per format and engine
(default, viterbi): one warm-up batch, then `repeats` timed ones — run_async + wait on the host clock (median, min, max) and the tile
kernel's duration from HIP events around it (lsdr_capture_batch_tile_time).  The cu8 rows come from the object made WITHOUT the new
arguments: on a checkout that has no other formats the tool reports those rows only, which is how the cu8 kernels are compared across
commits on one box.  Writes one JSON line to --out (default profiles/capture_batch_formats/bench.json) and to stdout."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_c1
import leansdr_amd.capi as capi

HAVE_FORMATS = "in_format" in inspect.signature(capi.CaptureBatch.__init__).parameters


def spread(ts):
    return dict(median=round(statistics.median(ts), 5), min=round(min(ts), 5), max=round(max(ts), 5), n=len(ts))


def convert(fmt, u):
    s = u.astype(np.int16) - 128
    if fmt == "cs8":
        return s.astype(np.int8), dict(in_format=capi.IN_CS8)
    if fmt == "cu16":
        return (s.astype(np.int32) * 256 + 32768).astype(np.uint16), dict(in_format=capi.IN_CU16, in_scale=2.0 ** -8)
    if fmt == "cs16":
        return (s.astype(np.int32) * 256).astype(np.int16), dict(in_format=capi.IN_CS16, in_scale=2.0 ** -8)
    if fmt == "cf32":
        return s.astype(np.float32) / np.float32(64), dict(in_format=capi.IN_CF32, in_scale=64.0)
    raise ValueError(fmt)


def timed(cb, ptrs, n, repeats):
    cb.tile_time(True)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        cb.run_async(ptrs, n)
        res = cb.wait()
        ts.append(time.perf_counter() - t0)
    tile_ms, launches = cb.tile_time(False)
    return ts, res, tile_ms, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=16)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--formats", default="cu8,cs8,cu16,cs16,cf32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_batch_formats", "bench.json"))
    args = ap.parse_args()
    B, n = args.captures, args.msamples << 20
    formats = [f for f in args.formats.split(",") if f == "cu8" or HAVE_FORMATS]
    ctx = capi.Ctx(0)
    gen = bench_c1.Generator(capi, ctx, n, B)
    cu8 = []
    for k in range(B):
        d, _ = gen.capture(k, 7000 + k)
        cu8.append(d)
    gen.close()
    rows, want = [], {}
    for fmt in formats:
        if fmt == "cu8":
            bufs, kw, own = cu8, {}, False
        else:
            bufs, own = [], True
            for d in cu8:
                items, kw = convert(fmt, ctx.download(d, np.uint8, 2 * n))
                bufs.append(ctx.upload(items))
        ptrs = [b.ptr for b in bufs]
        for engine, vit in (("default", None), ("viterbi", True)):
            cb = capi.CaptureBatch(ctx, B, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512, viterbi=vit, **kw)
            res, ts_bytes = cb.decode(ptrs, n)                 # warm-up; the TS is the cu8 object's
            if fmt == "cu8":
                want[engine] = ts_bytes
            same = ts_bytes == want.get(engine)
            ts, res, tile_ms, launches = timed(cb, ptrs, n, args.repeats)
            cb.close()
            row = dict(format=fmt, engine=engine, seconds_per_batch=spread(ts), msamples_per_s=round(B * n / statistics.median(ts) / 1e6, 1),
                       tile_kernel_ms=round(tile_ms, 3), tile_kernel_launches=launches, ts_packets=[r["ts_packets"] for r in res][:4],
                       locked=all(r["locked"] == 1 and r["seam_bad"] == 0 for r in res), ts_is_the_cu8_objects=bool(same))
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        if own:
            for b in bufs:
                b.free()
    for d in cu8:
        d.free()
    ctx.close()
    line = json.dumps(dict(tool="tools/capture_batch_formats_bench.py", workload=f"lsdr_capture_batch, B = {B} x {args.msamples} Mi samples, anf 1, tile_len 4096, "
                           "QPSK 1/2 at 1.2 samples per symbol, generator captures (Es/N0 as leanchansim --awgn 17.5)", repeats=args.repeats,
                           other_formats_in_this_checkout=HAVE_FORMATS, rows=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
