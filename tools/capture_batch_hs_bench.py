#!/usr/bin/env python3
"""tools/capture_batch_hs_bench.py [--captures 16,32] [--msamples 8] [--repeats 5] [--per-capture-runs 3] [--no-baselines] [--out FILE]

lsdr_hs_batch (`leandvb --u8 --hs` per capture) on one GPU, generator captures at the bench condition (bench_c1.Generator: QPSK 1/2,
1.2 samples per symbol, leanchansim --awgn 17.5), B captures of `msamples` Mi samples.  In ONE process:

  * the batch: run_async + wait on the host clock, one warm-up batch then `repeats` timed ones (median, min, max), and the host time spent
    inside run_async (a small fraction of the batch unless something synchronises);
  * the way to do the same job without it: bench_more.c1_hs called as is — per-capture FastQpsk(tiled) + HsDeconv + the block chain, every
    block returning its counts to the host, on 8 decoder threads — `per-capture-runs` times (each run is its own mean over at least
    bench_more.MIN_SECONDS);
  * optionally the reference: oracle/_ref/leandvb --hs on one host core, capture 0.

Every TS of the batch is checked before the clock starts: locked, and every packet behind the first 16 a transmitted one, in order.
`batch_slowest_beats_per_capture_fastest` compares the batch's slowest repeat with the per-capture path's fastest run.
Kernel times come from a run of this tool under `rocprofv3 --kernel-trace --stats` (with --no-baselines), not from here.
Writes one JSON line to --out (default profiles/hs_batch/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_c1
import bench_more
import leansdr_amd.capi as capi
from leansdr_amd import synth

REF_ARGS = ["--u8", "-f", "2400e3", "--sr", "2000e3", "--cr", "1/2", "--hs"]


def spread(ts):
    return dict(median=round(statistics.median(ts), 5), min=round(min(ts), 5), max=round(max(ts), 5), n=len(ts))


def check_ts(ts, sent, first_pk):
    pk = [ts[i:i + 188] for i in range(0, len(ts), 188)]
    if len(pk) <= 100:
        return False
    idx = [i for i in range(max(0, first_pk - 64), min(len(sent), first_pk + 4096)) if bytes(sent[i]) == pk[bench_c1.SKIP_ACQ]]
    return bool(idx) and b"".join(pk[bench_c1.SKIP_ACQ:]) == sent[idx[0]:idx[0] + len(pk) - bench_c1.SKIP_ACQ].tobytes()


def one_case(ctx, B, n, args):
    gen = bench_c1.Generator(capi, ctx, n, B)
    bufs, firsts = [], []
    for k in range(B):
        d, f = gen.capture(k, 7000 + k)
        bufs.append(d); firsts.append(f)
    sent = gen.ts
    gen.close()
    ptrs = [b.ptr for b in bufs]
    hb = capi.HsBatch(ctx, B, n, bench_c1.OMEGA, fastlock=args.fastlock, tile_len=args.tile_len, tile_warmup=args.tile_warmup)
    res, ts_bytes = hb.decode(ptrs, n)                   # warm-up (first launch of every kernel) and the check
    ok = all(r["locked"] == 1 and r["seam_bad"] == 0 for r in res) and all(check_ts(t, sent, f) for t, f in zip(ts_bytes, firsts))
    ts, host = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        hb.run_async(ptrs, n)
        t1 = time.perf_counter()
        res = hb.wait()
        ts.append(time.perf_counter() - t0)
        host.append(t1 - t0)
    hb.close()
    out = dict(captures=B, samples_per_capture=n,
               batch=dict(seconds_per_batch=spread(ts), run_async_host_seconds=spread(host),
                          run_async_share_of_batch=round(statistics.median(host) / statistics.median(ts), 4),
                          msamples_per_s=round(B * n / statistics.median(ts) / 1e6, 1),
                          msamples_per_s_range=[round(B * n / max(ts) / 1e6, 1), round(B * n / min(ts) / 1e6, 1)],
                          tiles_per_capture=res[0]["tiles"], ts_packets=[r["ts_packets"] for r in res][:4],
                          seams=dict(dup=sum(r["seam_dup"] for r in res), miss=sum(r["seam_miss"] for r in res), bad=sum(r["seam_bad"] for r in res)),
                          verified_against_transmitted_packets=bool(ok)))
    ref = os.path.join(ROOT, "oracle", "_ref", "leandvb")
    if args.cpu and os.access(ref, os.X_OK):
        iq = ctx.download(bufs[0], np.uint8, 2 * n).tobytes()
        t0 = time.perf_counter()
        r = subprocess.run([ref] + REF_ARGS, input=iq, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=900)
        dt = time.perf_counter() - t0
        out["reference_one_core"] = dict(command="oracle/_ref/leandvb " + " ".join(REF_ARGS), samples=n, seconds=round(dt, 2),
                                         msamples_per_s=round(n / dt / 1e6, 2), ts_packets=len(r.stdout) // 188)
    for b in bufs:
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", default="16,32")
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--per-capture-runs", type=int, default=3)
    ap.add_argument("--fastlock", type=int, default=0)
    ap.add_argument("--tile-len", type=int, default=0)
    ap.add_argument("--tile-warmup", type=int, default=0)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--cpu", action="store_true", help="also time oracle/_ref/leandvb --hs on one host core (capture 0 of the first case)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hs_batch", "bench.json"))
    args = ap.parse_args()
    ctx = capi.Ctx(0)
    cases = []
    for B in [int(x) for x in args.captures.split(",")]:
        c = one_case(ctx, B, args.msamples << 20, args)
        args.cpu = False
        cases.append(c)
        print(json.dumps(c), file=sys.stderr, flush=True)
    ctx.close()
    doc = dict(tool="tools/capture_batch_hs_bench.py", workload="lsdr_hs_batch, QPSK 1/2 at 1.2 samples per symbol, generator captures (Es/N0 as "
               "leanchansim --awgn 17.5), default tiles" if not args.tile_len else f"lsdr_hs_batch, tile_len {args.tile_len}",
               tile_kernel_lds_rect=os.environ.get("LSDR_HSB_LDS_RECT", "") or "by run size", repeats=args.repeats, cases=cases)
    if not args.no_baselines:
        runs = []
        for _ in range(args.per_capture_runs):
            r = bench_more.c1_hs_entry(capi, synth, 0, argparse.Namespace(tile_warmup=512))
            runs.append(dict(msamples_per_s=r["value"], seconds=r["seconds"], decoders=r["decoders"], verified=bool(r["pass"])))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
        rates = [r["msamples_per_s"] for r in runs]
        doc["per_capture_path"] = dict(what="bench_more.c1_hs as is: FastQpsk(tiled) + HsDeconv + block chain per capture, 8 decoder threads",
                                       runs=runs, msamples_per_s=dict(median=statistics.median(rates), min=min(rates), max=max(rates)))
        last = cases[-1]["batch"]
        doc["batch_slowest_beats_per_capture_fastest"] = dict(captures=cases[-1]["captures"], batch_slowest_msamples_per_s=last["msamples_per_s_range"][0],
                                                             per_capture_fastest_msamples_per_s=max(rates),
                                                             holds=bool(last["msamples_per_s_range"][0] > max(rates)))
    line = json.dumps(doc)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
