#!/usr/bin/env python3
"""tools/capture_batch_reports_bench.py [--captures 16] [--msamples 8] [--repeats 5] [--rounds 3] [--period 480000] [--parent-root DIR] [--out FILE]

What the capture batch's signal reports cost (lsdr_capture_reports_set), one GPU: B generator captures at the bench condition
(bench_c1.Generator: QPSK 1/2, 1.2 samples per symbol, leanchansim --awgn 17.5) of `msamples` Mi samples, cu8, anf 1, tile_len 4096, on
both engines.  Per engine two objects, reports off and reports on (period 480 000 samples: leandvb's default Finfo at 2.4 MS/s), timed
ALTERNATING in one process: `rounds` times [off: `repeats` batches, on: `repeats` batches], the tile kernel's duration from HIP events
around it (lsdr_capture_batch_tile_time) and run_async + wait on the host clock.  The reports-on object must return the reports-off
object's results and TS (checked before the clock starts); each capture's last SS / MER / FREQ is printed.

--parent-root DIR: a built checkout of the parent commit.  The same measurement (reports off: all it has) is then run on it too, in
processes that alternate with this checkout's — `rounds` processes each — and the result holds both tile times, both run_async + wait
times and the parent's run-to-run spread: an object without reports launches the kernels it launched there.

Writes one JSON line to --out (default profiles/capture_batch_reports/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(ts):
    return dict(median=round(statistics.median(ts), 5), min=round(min(ts), 5), max=round(max(ts), 5), n=len(ts))


def timed(cb, ptrs, n, repeats):
    cb.tile_time(True)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        cb.run_async(ptrs, n)
        cb.wait()
        ts.append(time.perf_counter() - t0)
    tile_ms, _ = cb.tile_time(False)
    return ts, tile_ms


def measure(root, args):
    """One process's measurement on the checkout at `root`: rows per engine."""
    sys.path.insert(0, root)
    import inspect
    import bench_c1
    import leansdr_amd.capi as capi
    have = "reports" in inspect.signature(capi.CaptureBatch.__init__).parameters
    B, n = args.captures, args.msamples << 20
    ctx = capi.Ctx(0)
    gen = bench_c1.Generator(capi, ctx, n, B)
    bufs = [gen.capture(k, 7000 + k)[0] for k in range(B)]
    gen.close()
    ptrs = [b.ptr for b in bufs]
    rows = []
    for engine, vit in (("default", None), ("viterbi", True)):
        objs = {"off": capi.CaptureBatch(ctx, B, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512, viterbi=vit)}
        if have:
            objs["on"] = capi.CaptureBatch(ctx, B, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512, viterbi=vit, reports=args.period)
        first = {k: cb.decode(ptrs, n) for k, cb in objs.items()}               # warm-up
        row = dict(engine=engine, locked=all(r["locked"] == 1 and r["seam_bad"] == 0 for r in first["off"][0]),
                   ts_packets=[r["ts_packets"] for r in first["off"][0]][:4])
        if have:
            row["reports_on_returns_the_reports_off_results_and_ts"] = bool(first["on"] == first["off"])
            last = [objs["on"].reports(i) for i in range(B)]
            row["reports_per_capture"] = int(len(last[0]["ss"]))
            row["last"] = [dict(freq=float(r["last"][0]), ss=round(float(r["last"][1]), 3), mer=round(float(r["last"][2]), 3)) for r in last]
            for i, r in enumerate(row["last"]):
                print(f"{engine} capture {i}: SS {r['ss']:.2f} MER {r['mer']:.2f} dB FREQ {r['freq']:+.3e}", file=sys.stderr, flush=True)
        tile = {k: [] for k in objs}
        wall = {k: [] for k in objs}
        for _ in range(args.rounds):
            for k, cb in objs.items():
                ts, ms = timed(cb, ptrs, n, args.repeats)
                tile[k].append(ms); wall[k] += ts
        for k, cb in objs.items():
            cb.close()
            row[f"tile_kernel_ms_{k}"] = dict(rounds=[round(v, 4) for v in tile[k]], median=round(statistics.median(tile[k]), 4))
            row[f"seconds_per_batch_{k}"] = spread(wall[k])
        if have:
            row["tile_kernel_on_over_off"] = round(row["tile_kernel_ms_on"]["median"] / row["tile_kernel_ms_off"]["median"], 4)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    for b in bufs:
        b.free()
    ctx.close()
    return rows


def child(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child-root", root, "--captures", str(args.captures), "--msamples", str(args.msamples),
           "--repeats", str(args.repeats), "--rounds", str(args.rounds), "--period", str(args.period)]
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
    ap.add_argument("--period", type=int, default=480000)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child-root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE_ROOT, "profiles", "capture_batch_reports", "bench.json"))
    args = ap.parse_args()
    if args.child_root:
        print(json.dumps(measure(args.child_root, args)))
        return
    result = dict(tool="tools/capture_batch_reports_bench.py",
                  workload=f"lsdr_capture_batch, B = {args.captures} x {args.msamples} Mi samples cu8, anf 1, tile_len 4096, QPSK 1/2 at 1.2 samples per "
                           "symbol, generator captures (Es/N0 as leanchansim --awgn 17.5)", report_period_samples=args.period, repeats=args.repeats,
                  rounds=args.rounds)
    if not args.parent_root:
        result["rows"] = measure(HERE_ROOT, args)
    else:
        # processes of the two checkouts alternating: [this, parent] × rounds; the first process of this checkout supplies the rows
        this, parent = [], []
        for _ in range(args.rounds):
            this.append(child(HERE_ROOT, args))
            parent.append(child(os.path.abspath(args.parent_root), args))
        result["rows"] = this[0]
        cmp_ = []
        for e, row in enumerate(this[0]):
            t = [r[e]["tile_kernel_ms_off"]["median"] for r in this]
            p = [r[e]["tile_kernel_ms_off"]["median"] for r in parent]
            cmp_.append(dict(engine=row["engine"], tile_kernel_ms_reports_off=dict(per_process=t, median=round(statistics.median(t), 4)),
                             tile_kernel_ms_parent=dict(per_process=p, median=round(statistics.median(p), 4)),
                             parent_run_to_run_spread_ms=round(max(p) - min(p), 4),
                             parent_round_to_round_spread_ms=round(max(max(r[e]["tile_kernel_ms_off"]["rounds"]) - min(r[e]["tile_kernel_ms_off"]["rounds"]) for r in parent), 4),
                             difference_ms=round(statistics.median(t) - statistics.median(p), 4),
                             seconds_per_batch_reports_off=[r[e]["seconds_per_batch_off"] for r in this],
                             seconds_per_batch_parent=[r[e]["seconds_per_batch_off"] for r in parent]))
        result["against_the_parent_commit"] = cmp_
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
