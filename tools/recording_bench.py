#!/usr/bin/env python3
"""tools/recording_bench.py [--streams 32] [--packets 68489] [--msamples 128] [--piece-msamples 16] [--repeats 5] [--out FILE]

What decoding a long recording in pieces costs, one GPU.

  * the stitch alone (lsdr_ts_stitch_run_async → lsdr_ts_stitch_wait, the C calls): `streams` streams of `packets` packets, windows of one
    long stream that overlap by 4096 packets (W = 4096, M = 8), beside their bytes over 8 TB/s;
  * RecordingDecoder.decode of one cu8 capture of `msamples` Mi samples (QPSK 1/2 at 1.2 samples per symbol, bench_c1.Generator) in pieces
    of `piece-msamples` Mi samples overlapping by overlap_for(FEC12, omega), beside the same capture as the one entry of a CaptureBatch of
    its whole length — the only way without pieces;
  * RecordingDecoder.decode_file of the same samples in a file, beside oracle/_ref/leandvb reading that file (skipped, and said so, where
    the binary is missing).

Writes one JSON line to --out (default profiles/recording/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
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
    ap.add_argument("--packets", type=int, default=68489)
    ap.add_argument("--msamples", type=int, default=128)
    ap.add_argument("--piece-msamples", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recording", "bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_c1
    import leansdr_amd.capi as capi
    import ts_batch_bench
    P, n, W = args.streams, args.packets, 4096
    ctx = capi.Ctx(0)
    result = dict(tool="tools/recording_bench.py", repeats=args.repeats)

    # ---- the stitch alone
    stride = n - W
    long = ts_batch_bench.build(stride * (P - 1) + n, 100)
    bufs = [ctx.upload(long[k * stride:k * stride + n]) for k in range(P)]
    st = capi.TsStitch(ctx, P, n, window=W, min_run=8)
    ptrs, lengths = [b.ptr for b in bufs], [n] * P

    def run():
        st.run_async(ptrs, lengths)
        capi.check(capi.lib.lsdr_ts_stitch_wait(st.h, st._joins, st._keep))
    joins, keep = st.stitch_records(ptrs, lengths)                         # warm-up, and the one condition: every pair joins over the overlap
    assert all(j["joined"] and j["run"] == W for j in joins) and st.packets == len(long), (joins[:2], st.packets)
    t = timed(run, args.repeats)
    result["stitch"] = dict(streams=P, packets=n, window=W, in_bytes=P * n * 188, out_bytes=st.packets * 188, seconds=spread(t),
                            # (the gather reads every kept byte and writes it: twice the output's bytes)
                            gather_bytes_over_8TBps_seconds=float(f"{2 * st.packets * 188 / HBM_BYTES_PER_S:.3e}"))
    t0 = time.perf_counter()
    st.download()
    result["stitch"]["download_seconds_once"] = round(time.perf_counter() - t0, 6)
    st.close()
    for b in bufs:
        b.free()

    # ---- one long capture: in pieces, and as one entry of a batch
    ns, piece = args.msamples << 20, args.piece_msamples << 20
    overlap = capi.overlap_for(capi.FEC12, bench_c1.OMEGA)
    gen = bench_c1.Generator(capi, ctx, ns, 1)
    cap = gen.capture(0, 7000)[0]
    gen.close()
    B = min(16, len(capi.recording_plan(ns, piece, overlap)))
    dec = capi.RecordingDecoder(ctx, piece, overlap, B, bench_c1.OMEGA, tune=0.0)
    ts, report = dec.decode(cap.ptr, ns)                                   # warm-up
    t_pieces = timed(lambda: dec.decode(cap.ptr, ns), args.repeats)
    result["decode_in_pieces"] = dict(msamples=args.msamples, piece_msamples=args.piece_msamples, overlap_samples=overlap, pieces=len(report["pieces"]),
                                      pieces_per_batch=B, seconds=spread(t_pieces), packets=report["packets"], unjoined=report["unjoined"],
                                      runs=[j["run"] for j in report["joins"]][:4],
                                      msamples_per_second=round(ns / statistics.median(t_pieces) / 1e6, 1))
    cb = capi.CaptureBatch(ctx, 1, ns, bench_c1.OMEGA)
    res, whole = cb.decode([cap.ptr], ns)                                  # warm-up
    t_whole = timed(lambda: cb.decode([cap.ptr], ns), args.repeats)
    cb.close()
    wpk, pk = [whole[0][i:i + 188] for i in range(0, len(whole[0]), 188)], [ts[i:i + 188] for i in range(0, len(ts), 188)]
    i0 = pk.index(wpk[16])
    m = min(len(pk) - i0, len(wpk) - 16)
    result["decode_whole"] = dict(seconds=spread(t_whole), packets=res[0]["ts_packets"], msamples_per_second=round(ns / statistics.median(t_whole) / 1e6, 1),
                                  same_packets_from_16_on=bool(pk[i0:i0 + m] == wpk[16:16 + m]), compared=m)
    result["pieces_over_whole"] = round(statistics.median(t_pieces) / statistics.median(t_whole), 3)

    # ---- the same samples in a file
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "capture.cu8")
        ctx.download(cap, np.uint8, 2 * ns).tofile(path)
        got, _ = dec.decode_file(path)                                     # warm-up (the page cache holds the file from here on)
        t_file = timed(lambda: dec.decode_file(path), args.repeats)
        result["decode_file"] = dict(seconds=spread(t_file), same_bytes_as_decode=bool(got == ts),
                                     msamples_per_second=round(ns / statistics.median(t_file) / 1e6, 1))
        if os.access(bench_c1.REFBIN, os.X_OK):
            t0 = time.perf_counter()
            with open(path, "rb") as f:
                ref = subprocess.run([bench_c1.REFBIN] + bench_c1.REF_ARGS_BASE, stdin=f, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
            t_ref = time.perf_counter() - t0
            result["reference_leandvb"] = dict(seconds_once=round(t_ref, 3), packets=len(ref) // 188, msamples_per_second=round(ns / t_ref / 1e6, 2))
            result["reference_over_decode_file"] = round(t_ref / statistics.median(t_file), 1)
        else:
            result["reference_leandvb"] = "oracle/_ref/leandvb is missing: not measured"
    dec.close()
    cap.free()
    ctx.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
