#!/usr/bin/env python3
"""tools/carrier_scan_bench.py [--captures 32] [--msamples 8] [--repeats 9] [--inner 20] [--out FILE]

What finding the carriers of every capture (lsdr_carrier_scan) costs, one GPU, cu8: B captures of `msamples` Mi samples, each the sum of
three DVB-S carriers (12, 8 and 24 samples per symbol) plus noise — tests/scan_common.py's mix A, one capture made on the host and
uploaded B times.  After one warm-up each, `repeats` samples of `inner` calls on the host clock, in one process, the objects taking
turns sample by sample (every timed call ends in a wait):

  * the carrier scan, run_async → wait, with 64 and with 256 blocks of 4096 samples per capture, spread over the capture;
  * the rate estimator (lsdr_rate_est) at the same block counts: the same loads and transforms, a row half as long, no sort;
  * the scan's bytes — per block its samples read, its row of 4096 floats written and read again — over 8 TB/s, beside its time;
  * WidebandDecoder.decode on the two-carrier capture of tests/test_gpu_carrier_scan.py's closed loop (6 267 071 samples), split into
    its steps (capi.WidebandDecoder.steps: each step makes its objects, runs them and ends in a wait).

The figures are recorded, no threshold is set.

Writes one JSON line to --out (default profiles/carrier_scan/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12


def spread(ts):
    return dict(median=round(statistics.median(ts), 7), min=round(min(ts), 7), max=round(max(ts), 7), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=32)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carrier_scan", "bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import leansdr_amd.capi as capi
    import scan_common as sc
    B, n = args.captures, args.msamples << 20
    ctx = capi.Ctx(0)
    iq = sc.mix(tuple(sc.MIX_A), n, 7.5, 1)
    bufs = [ctx.upload(iq) for _ in range(B)]
    ptrs, lengths = [b.ptr for b in bufs], [n] * B
    result = dict(tool="tools/carrier_scan_bench.py", repeats=args.repeats, inner=args.inner,
                  workload=f"B = {B} x {args.msamples} Mi samples cu8, three carriers (12, 8, 24 samples per symbol) plus noise 7.5; seconds per call")
    for blocks in (64, 256):
        scan = capi.CarrierScan(ctx, B, blocks=blocks)
        rate = capi.RateEstimator(ctx, B, blocks=blocks)
        got = scan.scan(ptrs, lengths)                                          # warm-up
        rate.estimate(ptrs, lengths)
        ts = {"scan": [], "rate": []}
        for _ in range(args.repeats):
            for name, fn in (("scan", lambda: scan.scan(ptrs, lengths)), ("rate", lambda: rate.estimate(ptrs, lengths))):
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    fn()
                ts[name].append((time.perf_counter() - t0) / args.inner)
        scan.close()
        rate.close()
        M = got[0]["blocks"]
        nbytes = B * M * (4096 * 2 + 2 * 4096 * 4)
        s, r = statistics.median(ts["scan"]), statistics.median(ts["rate"])
        result[f"{blocks}_blocks"] = dict(
            carrier_scan_seconds=spread(ts["scan"]), rate_estimator_seconds=spread(ts["rate"]), scan_over_rate=round(s / r, 4),
            scan_bytes=nbytes, scan_bytes_over_8TBps_seconds=round(nbytes / HBM_BYTES_PER_S, 7), scan_over_bytes_bound=round(s / (nbytes / HBM_BYTES_PER_S), 2),
            blocks=M, stride=got[0]["stride"], found=[g["found"] for g in got][:2],
            carriers=[[round(c["center"], 5), round(c["omega"], 3), round(c["cnr_db"], 2)] for c in got[0]["carriers"]])
    for b in bufs:
        b.free()
    wide = sc.wideband()
    buf = ctx.upload(wide)
    dec = capi.WidebandDecoder(ctx, sc.WIDE_N)
    scan, carriers = dec.decode(buf.ptr, sc.WIDE_N)                             # warm-up
    steps, total = {}, []
    for _ in range(max(3, args.repeats // 2)):
        t0 = time.perf_counter()
        dec.decode(buf.ptr, sc.WIDE_N)
        total.append(time.perf_counter() - t0)
        for k, v in dec.steps.items():
            steps.setdefault(k, []).append(v)
    buf.free()
    result["wideband_decode"] = dict(
        samples=sc.WIDE_N, seconds=spread(total), steps={k: spread(v) for k, v in steps.items()},
        carriers=[dict(center=round(c["center"], 5), omega_scan=round(c["omega_scan"], 3), decim=c["decim"], omega=c["omega"] and round(c["omega"], 5),
                       tune=c["tune"] and round(c["tune"], 6), ts_packets=len(c["ts"]) // 188) for c in carriers])
    ctx.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
