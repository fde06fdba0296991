#!/usr/bin/env python3
"""tools/capture_batch_relock_bench.py [--captures 32] [--msamples 8] [--repeats 7] [--parent-root DIR] [--out FILE] [--packets FILE]

What re-acquisition (lsdr_capture_relock_set) costs and returns, one GPU: B generator captures at the bench condition (bench_c1.Generator:
QPSK 1/2, 1.2 samples per symbol, leanchansim --awgn 17.5) of `msamples` Mi samples, anf 1, tile_len 4096; run_async to wait on the host
clock, one warm-up batch, then `repeats` timed ones (median, min, max).

  clean     the captures as generated with relock 0, 1, 3 and 8: the price of the passes that find nothing to do;
  burst     the same captures with n/40 samples of garbage from n/2 on and everything behind the middle of the burst turned by 180 degrees,
            relock 0 against 3: the rest-of-capture search by one workgroup against a whole-chip stretch, and the packets returned;
  parent    with --parent-root DIR (a built checkout of the parent commit): the clean captures with relock off, in fresh processes —
            parent, this checkout, parent — so that the parent's own spread from run to run is on record beside the difference.

--packets FILE (default profiles/capture_batch_relock/packets.txt; "" to skip): 2500-packet captures of tests/batch_common.rate_capture
with a step behind a burst (tests/relock_common.single_step) — the batch's TS packets with relock 0 and 3, and the reference binary's
(oracle/_ref/leandvb --anf 0) beside them where it is built.  Recorded, not compared: the reference's own count varies from run to run.
Writes one JSON line to --out (default profiles/capture_batch_relock/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(ts):
    return dict(median=round(statistics.median(ts), 5), min=round(min(ts), 5), max=round(max(ts), 5), n=len(ts))


def timed(cb, ptrs, n, repeats):
    cb.run_async(ptrs, n)
    cb.wait()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        cb.run_async(ptrs, n)
        res = cb.wait()
        ts.append(time.perf_counter() - t0)
    return ts, res


def stepped(u, n):
    """n/40 samples of garbage from n/2 on, everything behind the middle of the burst turned by 180 degrees (x -> 255 - x on the cu8 grid)."""
    burst, out = n // 40, u.copy()
    out[2 * (n // 2): 2 * (n // 2 + burst)] = np.random.default_rng(5).integers(100, 156, 2 * burst, dtype=np.uint8)
    mid = n // 2 + burst // 2
    out[2 * mid:] = 255 - out[2 * mid:]
    return out


def measure(root, B, n, repeats, what):
    """Rows of `what` ("clean0": relock off only, through the constructor every checkout has; "all") with the library of checkout `root`."""
    sys.path.insert(0, root)
    import bench_c1
    import leansdr_amd.capi as capi
    ctx = capi.Ctx(0)
    gen = bench_c1.Generator(capi, ctx, n, B)
    clean = [gen.capture(k, 7000 + k)[0] for k in range(B)]
    gen.close()
    rows = []

    def row(name, bufs, relock):
        cb = capi.CaptureBatch(ctx, B, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512)
        if relock:
            cb.set_relock(relock)
        ts, res = timed(cb, [b.ptr for b in bufs], n, repeats)
        r = dict(captures=name, relock=relock, seconds_per_batch=spread(ts), msamples_per_s=round(B * n / statistics.median(ts) / 1e6, 1),
                 ts_packets=sum(r["ts_packets"] for r in res), locked=sum(r["locked"] for r in res))
        if relock:
            st = [cb.relock_stats(i) for i in range(B)]
            r.update(passes=max(s["passes"] for s in st), exhausted=sum(s["exhausted"] for s in st), locks=sum(s["locks"] for s in st))
        cb.close()
        rows.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)

    row("clean", clean, 0)
    if what == "all":
        for relock in (1, 3, 8):
            row("clean", clean, relock)
        burst = [ctx.upload(stepped(ctx.download(d, np.uint8, 2 * n), n)) for d in clean]
        for relock in (0, 3):
            row("burst and a step of 180 degrees at n/2", burst, relock)
        for b in burst:
            b.free()
    for d in clean:
        d.free()
    ctx.close()
    return rows


def child(root, args):
    """measure(root, …, "clean0") in a fresh process: one JSON line on its standard output."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", root, "--captures", str(args.captures), "--msamples", str(args.msamples),
                          "--repeats", str(args.repeats)], stdout=subprocess.PIPE, check=True, timeout=900).stdout
    return json.loads(out.decode().strip().splitlines()[-1])[0]


def packets_record(path):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.join(HERE, "oracle"))
    sys.path.insert(0, HERE)
    import bench_c1
    import leansdr_amd.capi as capi
    import relock_common as rc
    from batch_common import CR, REFBIN, rate_capture, ref_args, run_reference
    ctx = capi.Ctx(0)
    lines = ["tools/capture_batch_relock_bench.py: 2500-packet captures (batch_common.rate_capture, 1.2 samples per symbol, --awgn 17.5), n/40 samples of garbage from n/2 on,",
             "everything behind the middle of the burst turned by `step` degrees (relock_common.single_step); anf 0.  TS packets returned.",
             "The reference binary's count is not the same from run to run (its scheduler follows how its input arrived): recorded, not compared.",
             "rate step  relock0 locked  relock3 locked locks next_sync  reference"]
    for rate, steps in ((0, (0, 90, 180, 270)), (1, (90,)), (3, (180, 270)), (4, (90,)), (5, (180,))):
        base = rate_capture(rate, 2500)[0]
        for deg in steps:
            iq = rc.single_step(base, deg)
            n = len(iq) // 2
            buf = ctx.upload(iq)
            cb = capi.CaptureBatch(ctx, 1, n, bench_c1.OMEGA, fec=rate, anf=0)
            r0, _ = cb.decode([buf.ptr], n)
            cb.set_relock(3)
            r3, _ = cb.decode([buf.ptr], n)
            st = cb.relock_stats(0)
            cb.close(); buf.free()
            ref = len(run_reference(ref_args(rate, "--anf", "0"), iq)) // 188 if os.path.exists(REFBIN) else "-"
            lines.append(f"{CR[rate]:>4} {deg:>4}  {r0[0]['ts_packets']:>7} {r0[0]['locked']:>6}  {r3[0]['ts_packets']:>7} {r3[0]['locked']:>6} {st['locks']:>5} "
                         f"{r3[0]['next_sync_calls']:>9}  {ref:>9}")
            print(lines[-1], file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=32)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--child-root", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "capture_batch_relock", "bench.json"))
    ap.add_argument("--packets", default=os.path.join(HERE, "profiles", "capture_batch_relock", "packets.txt"))
    args = ap.parse_args()
    B, n = args.captures, args.msamples << 20
    if args.child_root:
        print(json.dumps(measure(args.child_root, B, n, args.repeats, "clean0")))
        return
    parent = None
    if args.parent_root:
        a = child(args.parent_root, args)
        here = child(HERE, args)
        b = child(args.parent_root, args)
        lo, hi = sorted((a["seconds_per_batch"]["median"], b["seconds_per_batch"]["median"]))
        parent = dict(order="parent, this checkout, parent: fresh processes, clean captures, relock off", parent_first=a, this_checkout=here, parent_again=b,
                      parent_spread_of_medians=round(hi - lo, 5),
                      this_minus_parent_mean=round(here["seconds_per_batch"]["median"] - (lo + hi) / 2, 5))
    rows = measure(HERE, B, n, args.repeats, "all")
    line = json.dumps(dict(tool="tools/capture_batch_relock_bench.py", workload=f"lsdr_capture_batch, B = {B} x {args.msamples} Mi samples, anf 1, tile_len 4096, "
                           "QPSK 1/2 at 1.2 samples per symbol, generator captures (Es/N0 as leanchansim --awgn 17.5), run_async to wait",
                           repeats=args.repeats, rows=rows, against_parent=parent))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.packets:
        packets_record(args.packets)


if __name__ == "__main__":
    main()
