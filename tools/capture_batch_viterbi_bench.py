#!/usr/bin/env python3
"""tools/capture_batch_viterbi_bench.py [--captures 16,32] [--msamples 8] [--repeats 5] [--no-baselines] [--out FILE]

The capture batch's Viterbi engine (`leandvb --u8 … --viterbi` per capture) on one GPU, generator captures at the bench condition
(bench_c1.Generator: QPSK 1/2, 1.2 samples per symbol, leanchansim --awgn 17.5), B captures of `msamples` Mi samples:

  * the batch: run_async + wait, host clock, one warm-up batch then `repeats` timed ones (median, min, max); the tile kernel's duration
    from HIP events around it (lsdr_capture_batch_tile_time); rounds of the Viterbi stage = host reads of B records per batch;
  * the DEFAULT engine (packed decisions, algebraic deconvolution) on the same captures: its whole job and its tile kernel — what the soft
    store and the cost arithmetic add to the tiles;
  * the way to do the same job without this engine: the unchanged leandvb.cc on the GPU blocks, one process per capture
    (`LSDR_TILED=1 oracle/_ref/ref_graph/leandvb … --viterbi --buf-factor 4096`), at most `--procs` at a time, the same IQ from files;
  * the reference: oracle/_ref/leandvb … --viterbi on one host core, the first 8 Mi samples of capture 0.

Every TS of the batch is checked before the clock starts: locked, and every packet behind the first 16 a transmitted one, in order.
Per-stage kernel times come from a run of this tool under `rocprofv3 --kernel-trace --stats` (with --no-baselines), not from here.
Writes one JSON line to --out (default profiles/capture_batch_viterbi/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_c1
import leansdr_amd.capi as capi

REF_ARGS = ["--u8", "-f", "2400e3", "--sr", "2000e3", "--cr", "1/2", "--viterbi"]


def spread(ts):
    return dict(median=round(statistics.median(ts), 5), min=round(min(ts), 5), max=round(max(ts), 5), n=len(ts))


def timed(cb, ptrs, n, repeats):
    cb.decode(ptrs, n)                                   # warm-up (first launch of every kernel, allocations)
    cb.tile_time(True)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        cb.run_async(ptrs, n)
        res = cb.wait()
        ts.append(time.perf_counter() - t0)
    tile_ms, launches = cb.tile_time(False)
    return ts, res, tile_ms, launches


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
    out = dict(captures=B, samples_per_capture=n)
    for name, vit in (("viterbi", True), ("default", None)):
        cb = capi.CaptureBatch(ctx, B, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512, viterbi=vit)
        res, ts_bytes = cb.decode(ptrs, n)
        ok = all(r["locked"] == 1 and r["seam_bad"] == 0 for r in res) and all(check_ts(t, sent, f) for t, f in zip(ts_bytes, firsts))
        ts, res, tile_ms, launches = timed(cb, ptrs, n, args.repeats)
        rep = dict(seconds_per_batch=spread(ts), msamples_per_s=round(B * n / statistics.median(ts) / 1e6, 1),
                   msamples_per_s_range=[round(B * n / max(ts) / 1e6, 1), round(B * n / min(ts) / 1e6, 1)],
                   tile_kernel_ms=round(tile_ms, 3), tile_kernel_launches=launches, ts_packets=[r["ts_packets"] for r in res][:4],
                   verified_against_transmitted_packets=bool(ok))
        if vit:
            st = [cb.viterbi_stats(i) for i in range(B)]
            rep.update(viterbi_rounds_per_batch=st[0]["batch_rounds"], host_reads_per_batch=st[0]["batch_rounds"] + 1,
                       rounds_per_capture=sorted({s["rounds"] for s in st}), switches=sum(s["switches"] for s in st), stalls=sum(s["stalls"] for s in st))
        out[name] = rep
        cb.close()
    if not args.no_baselines:
        tmp = tempfile.mkdtemp(prefix="cbv_")
        files = []
        for k, b in enumerate(bufs):
            p = os.path.join(tmp, f"cap{k}.cu8")
            ctx.download(b, np.uint8, 2 * n).tofile(p)
            files.append(p)
        graph = os.path.join(ROOT, "oracle", "_ref", "ref_graph", "leandvb")
        if os.access(graph, os.X_OK):
            env = dict(os.environ, LSDR_TILED="1")

            def proc(p):
                with open(p, "rb") as f:
                    r = subprocess.run([graph] + REF_ARGS + ["--buf-factor", "4096"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, timeout=900)
                return len(r.stdout) // 188, r.returncode
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=args.procs) as ex:
                got = list(ex.map(proc, files))
            dt = time.perf_counter() - t0
            out["per_capture_processes"] = dict(command="LSDR_TILED=1 oracle/_ref/ref_graph/leandvb " + " ".join(REF_ARGS) + " --buf-factor 4096",
                                                at_a_time=args.procs, seconds=round(dt, 2), msamples_per_s=round(B * n / dt / 1e6, 1),
                                                ts_packets=[g[0] for g in got][:4], exit_codes=sorted({g[1] for g in got}), passes=1)
        ref = os.path.join(ROOT, "oracle", "_ref", "leandvb")
        if os.access(ref, os.X_OK) and args.cpu:
            m = min(n, 8 << 20)
            iq = np.fromfile(files[0], np.uint8, 2 * m).tobytes()
            t0 = time.perf_counter()
            r = subprocess.run([ref] + REF_ARGS, input=iq, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=900)
            dt = time.perf_counter() - t0
            out["reference_one_core"] = dict(command="oracle/_ref/leandvb " + " ".join(REF_ARGS), samples=m, seconds=round(dt, 2),
                                             msamples_per_s=round(m / dt / 1e6, 2), ts_packets=len(r.stdout) // 188)
        for p in files:
            os.unlink(p)
        os.rmdir(tmp)
    for b in bufs:
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", default="16,32")
    ap.add_argument("--msamples", default="8")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--procs", type=int, default=12, help="per-capture processes at a time (this process holds the GPU too: 16 in all at most)")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--no-cpu", dest="cpu", action="store_false")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_batch_viterbi", "bench.json"))
    args = ap.parse_args()
    assert 1 <= args.procs <= 15
    ctx = capi.Ctx(0)
    cases = []
    cpu_done = False
    for ms in [int(x) for x in args.msamples.split(",")]:
        for B in [int(x) for x in args.captures.split(",")]:
            args.cpu = args.cpu and not cpu_done
            c = one_case(ctx, B, ms << 20, args)
            cpu_done = cpu_done or "reference_one_core" in c
            cases.append(c)
            print(json.dumps(c), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(dict(tool="tools/capture_batch_viterbi_bench.py", workload="lsdr_capture_batch, anf 1, tile_len 4096, QPSK 1/2 at 1.2 samples per symbol, "
                           "generator captures (Es/N0 as leanchansim --awgn 17.5)", repeats=args.repeats, cases=cases))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
