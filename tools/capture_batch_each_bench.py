#!/usr/bin/env python3
"""tools/capture_batch_each_bench.py [--captures 16] [--msamples 8] [--repeats 5] [--rounds 3] [--parent-root DIR] [--out FILE]

What per-capture lengths and tunes (lsdr_capture_each) cost, one GPU, generator captures at the bench condition (bench_c1.Generator:
QPSK 1/2, 1.2 samples per symbol, leanchansim --awgn 17.5), cu8, anf 1, tile_len 4096, both engines of lsdr_capture_batch and
lsdr_hs_batch.  Per process, after one warm-up batch each:

  * UNIFORM batches through the old entry points (B captures of `msamples` Mi samples): `repeats` batches, run_async + wait on the host
    clock, and for the capture batch the tile kernel's duration from HIP events around it (lsdr_capture_batch_tile_time);
  * a RAGGED job, B lengths spread evenly from 1 Mi to `msamples` Mi samples: one `each` batch, against the same B captures run as B
    uniform single-capture batches on one object per length (what a caller had to do before); both times and their ratio.  The each
    batch must return the single-capture runs' results and TS (checked before the clock starts).

--parent-root DIR: a built checkout of the parent commit.  The uniform measurement is then run on it too, in processes that alternate
with this checkout's — `rounds` processes each — and the result holds, per engine, both tile-kernel medians, both run_async + wait
medians, the parent's own min–max over its processes and whether this checkout's median lies inside it.

Writes one JSON line to --out (default profiles/capture_batch_each/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = (("default", None), ("viterbi", True))


def spread(ts):
    return dict(median=round(statistics.median(ts), 5), min=round(min(ts), 5), max=round(max(ts), 5), n=len(ts))


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def measure(root, args):
    """One process's measurement on the checkout at `root`."""
    sys.path.insert(0, root)
    import bench_c1
    import leansdr_amd.capi as capi
    have = hasattr(capi, "CaptureEach")
    B, n = args.captures, args.msamples << 20
    ctx = capi.Ctx(0)
    gen = bench_c1.Generator(capi, ctx, n, B)
    bufs = [gen.capture(k, 7000 + k)[0] for k in range(B)]
    gen.close()
    ptrs = [b.ptr for b in bufs]
    lengths = [(1 << 20) + (k * (n - (1 << 20))) // max(B - 1, 1) for k in range(B)]
    out = dict(uniform=[], ragged=[])

    def make(kind, n_captures, max_samples):
        if kind == "hs":
            return capi.HsBatch(ctx, n_captures, max_samples, bench_c1.OMEGA)
        return capi.CaptureBatch(ctx, n_captures, max_samples, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512, viterbi=dict(ENGINES)[kind])

    for kind in ("default", "viterbi", "hs"):
        cb = make(kind, B, n)
        first = cb.decode(ptrs, n)                                             # warm-up
        row = dict(engine=kind, locked=all(r["locked"] == 1 and r["seam_bad"] == 0 for r in first[0]), ts_packets=[r["ts_packets"] for r in first[0]][:4])
        if kind != "hs":
            cb.tile_time(True)
        ts = timed(lambda: (cb.run_async(ptrs, n), cb.wait()), args.repeats)
        if kind != "hs":
            row["tile_kernel_ms"] = round(cb.tile_time(False)[0], 4)
        row["seconds_per_batch"] = spread(ts)
        out["uniform"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        if have:
            singles = [make(kind, 1, L) for L in lengths]
            alone = [s.decode([ptrs[k]], lengths[k]) for k, s in enumerate(singles)]      # warm-up, and the yardstick
            got = cb.decode_each(ptrs, lengths)
            rag = dict(engine=kind, lengths_mi=[round(L / (1 << 20), 3) for L in lengths],
                       each_returns_the_single_capture_results_and_ts=all(got[0][k] == alone[k][0][0] and got[1][k] == alone[k][1][0] for k in range(B)))
            t_each = timed(lambda: (cb.run_each_async(ptrs, lengths), cb.wait()), args.repeats)

            def one_by_one():
                for k, s in enumerate(singles):
                    s.run_async([ptrs[k]], lengths[k])
                    s.wait()

            t_single = timed(one_by_one, args.repeats)
            rag["seconds_each_batch"] = spread(t_each)
            rag["seconds_single_capture_batches"] = spread(t_single)
            rag["single_over_each"] = round(statistics.median(t_single) / statistics.median(t_each), 3)
            rag["each_over_uniform_full_length"] = round(statistics.median(t_each) / statistics.median(ts), 3)
            for s in singles:
                s.close()
            out["ragged"].append(rag)
            print(json.dumps(rag), file=sys.stderr, flush=True)
        cb.close()
    for b in bufs:
        b.free()
    ctx.close()
    return out


def child(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child-root", root, "--captures", str(args.captures), "--msamples", str(args.msamples),
           "--repeats", str(args.repeats), "--rounds", str(args.rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
    if p.returncode:
        raise SystemExit(f"measurement process on {root} ended with {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=16)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child-root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE_ROOT, "profiles", "capture_batch_each", "bench.json"))
    args = ap.parse_args()
    if args.child_root:
        print(json.dumps(measure(args.child_root, args)))
        return
    result = dict(tool="tools/capture_batch_each_bench.py",
                  workload=f"B = {args.captures} x {args.msamples} Mi samples cu8, anf 1, tile_len 4096 (lsdr_capture_batch, both engines) and lsdr_hs_batch, "
                           "QPSK 1/2 at 1.2 samples per symbol, generator captures (Es/N0 as leanchansim --awgn 17.5); ragged: lengths spread evenly "
                           f"from 1 Mi to {args.msamples} Mi samples", repeats=args.repeats, rounds=args.rounds)
    if not args.parent_root:
        m = measure(HERE_ROOT, args)
        result["uniform"], result["ragged"] = m["uniform"], m["ragged"]
    else:
        # processes of the two checkouts alternating: [this, parent] × rounds; the first process of this checkout supplies the rows
        this, parent = [], []
        for _ in range(args.rounds):
            this.append(child(HERE_ROOT, args))
            parent.append(child(os.path.abspath(args.parent_root), args))
        result["uniform"], result["ragged"] = this[0]["uniform"], this[0]["ragged"]
        cmp_ = []
        for e, row in enumerate(this[0]["uniform"]):
            key = "tile_kernel_ms" if "tile_kernel_ms" in row else None
            c = dict(engine=row["engine"])
            if key:
                t, p = [r["uniform"][e][key] for r in this], [r["uniform"][e][key] for r in parent]
                c.update(tile_kernel_ms=dict(per_process=t, median=round(statistics.median(t), 4)),
                         tile_kernel_ms_parent=dict(per_process=p, median=round(statistics.median(p), 4), min=min(p), max=max(p)),
                         tile_kernel_median_inside_the_parents_min_max=bool(min(p) <= statistics.median(t) <= max(p)),
                         tile_kernel_median_over_parent_median=round(statistics.median(t) / statistics.median(p), 4))
            t = [r["uniform"][e]["seconds_per_batch"]["median"] for r in this]
            p = [r["uniform"][e]["seconds_per_batch"]["median"] for r in parent]
            c.update(seconds_per_batch=dict(per_process=t, median=round(statistics.median(t), 5)),
                     seconds_per_batch_parent=dict(per_process=p, median=round(statistics.median(p), 5), min=min(p), max=max(p)),
                     seconds_per_batch_median_inside_the_parents_min_max=bool(min(p) <= statistics.median(t) <= max(p)),
                     seconds_per_batch_median_over_parent_median=round(statistics.median(t) / statistics.median(p), 4))
            cmp_.append(c)
        result["uniform_against_the_parent_commit"] = cmp_
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
