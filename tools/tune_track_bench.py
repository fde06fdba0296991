#!/usr/bin/env python3
"""tools/tune_track_bench.py [--captures 32] [--msamples 8] [--recording-msamples 128] [--repeats 3] [--out FILE] [--accuracy FILE]

What following a carrier that moves costs, one GPU, generator captures at the bench condition (bench_c1.Generator: QPSK 1/2, 1.2 samples
per symbol, leanchansim --awgn 17.5), cu8.  After one warm-up each, medians of `repeats` on the host clock, every timed call ending in a
wait:

  * the tracker alone (lsdr_tune_track, hop 65536, 4 blocks per frame) beside TuneEstimator(blocks=64);
  * the derotator alone (lsdr_derotate_batch, the tracker's knots) beside its bytes over 8 TB/s: 2 read and 8 written per cu8 sample;
  * TrackedDecoder.decode in its three steps, beside CaptureBatch(IN_CF32).decode_each on the derotated streams and the cu8
    CaptureBatch.decode_estimated on the same (undrifted) captures: the price of tracking;
  * RecordingDecoder(tune="pieces") beside tune=None on one capture of `recording-msamples` Mi samples (tools/recording_bench.py's shape).

--accuracy FILE (default profiles/tune_track/accuracy.txt; "" to skip): the track's error against the true offset and the smallest quality
per A, noise, hop and blocks on tests/track_common.py's drifted captures, from the float64 restatement and from the device.

Writes one JSON line to --out (default profiles/tune_track/bench.json) and to stdout."""
import argparse
import json
import os
import statistics
import sys
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


def accuracy(capi, ctx, path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import track_common as trk
    import tune_common as tc
    caps = [(noise, A, ph) for noise in (7.5, 18.0) for A, ph in ((1e-3, 0.0), (2e-3, 0.0), (2e-3, 1.0), (4e-3, 0.0))]
    data = [trk.drifted_capture(*c) for c in caps]
    bufs = [ctx.upload(iq) for iq, _ in data]
    n = len(data[0][1])
    lines = ["# track error max|track(n) - f(n)| over the whole capture (cycles per sample) and the smallest quality of the accepted frames;",
             "# capture(1000, 11, noise) with an offset of A sin(2 pi n / T + phase), T = the capture's length (1 958 423 samples), span 64, min_quality 30.",
             "# the tiles' window at 1.2 samples per symbol is 4.07e-4; the tests hold the restatement to a quarter of it (1.0e-4) at hop 65536, blocks 4.",
             "noise      A  phase     hop  blocks  frames  accepted   restatement: error  quality      device: error  quality"]
    for hop, blocks in ((65536, 4), (32768, 4), (131072, 4), (262144, 4), (65536, 2), (65536, 8)):
        tr = capi.TuneTracker(ctx, len(caps), blocks=blocks, hop=hop, max_frames=n // hop + 2)
        got = tr.track([b.ptr for b in bufs], [n] * len(caps))
        tr.close()
        for (noise, A, ph), (iq, f), g in zip(caps, data, got):
            w = trk.track(tc.to_complex(iq), blocks=blocks, hop=hop)
            ew = float(np.max(np.abs(trk.track_value(trk.knots_of(w["frames"]), n) - f)))
            eg = float(np.max(np.abs(trk.track_value(capi.track_knots(g["frames"]), n) - f)))
            lines.append(f"{noise:5.1f}  {A:.0e}  {ph:5.1f}  {hop:6d}  {blocks:6d}  {len(g['frames']):6d}  {g['accepted']:8d}   {ew:18.2e}  {w['quality_min']:7.0f}      {eg:13.2e}  {g['quality_min']:7.0f}")
    for b in bufs:
        b.free()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=32)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--recording-msamples", type=int, default=128)
    ap.add_argument("--piece-msamples", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tune_track", "bench.json"))
    ap.add_argument("--accuracy", default=os.path.join(ROOT, "profiles", "tune_track", "accuracy.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench_c1
    import leansdr_amd.capi as capi
    B, n, R = args.captures, args.msamples << 20, args.repeats
    ctx = capi.Ctx(0)
    if args.accuracy:
        accuracy(capi, ctx, args.accuracy)
    gen = bench_c1.Generator(capi, ctx, n, B)
    bufs = [gen.capture(k, 7000 + k)[0] for k in range(B)]
    gen.close()
    ptrs, lengths = [b.ptr for b in bufs], [n] * B
    result = dict(tool="tools/tune_track_bench.py", repeats=R,
                  workload=f"B = {B} x {args.msamples} Mi samples cu8, QPSK 1/2 at 1.2 samples per symbol, generator captures (Es/N0 as leanchansim --awgn 17.5), "
                           "carrier at rest; capture batches: default engine, anf 1, tile_len 4096")

    # ---- the tracker alone, beside the estimator with 64 blocks
    td = capi.TrackedDecoder(ctx, B, n, bench_c1.OMEGA, anf=1, batch_kw=dict(tile_len=4096, tile_warmup=512))
    tracks = td.tracker.track(ptrs, lengths)
    t = timed(lambda: td.tracker.track(ptrs, lengths), R)
    result["tracker"] = dict(seconds=spread(t), hop=65536, blocks=4, frames=len(tracks[0]["frames"]), accepted=min(x["accepted"] for x in tracks),
                             max_abs_tune=max(max(abs(x["tune_min"]), abs(x["tune_max"])) for x in tracks),
                             min_quality=round(min(x["quality_min"] for x in tracks), 1), blocks_transformed=B * len(tracks[0]["frames"]) * 4)
    est = capi.TuneEstimator(ctx, B, blocks=64)
    est.estimate(ptrs, lengths)
    t64 = timed(lambda: est.estimate(ptrs, lengths), R)
    est.close()
    result["estimator_64_blocks"] = dict(seconds=spread(t64), blocks_transformed=B * 64)

    # ---- the derotator alone
    knots = [capi.track_knots(x["frames"]) for x in tracks]
    outs = [b.ptr for b in td._outs]
    td.derotator.run(ptrs, lengths, knots, outs)
    t = timed(lambda: td.derotator.run(ptrs, lengths, knots, outs), R)
    nbytes = B * n * 10
    result["derotator"] = dict(seconds=spread(t), knots=len(knots[0]), bytes=nbytes, bytes_over_8TBps_seconds=float(f"{nbytes / HBM_BYTES_PER_S:.3e}"),
                               GBps=round(nbytes / statistics.median(t) / 1e9, 1))

    # ---- the decode: tracked, its cf32 decode alone, and the cu8 decode with one estimated tune
    res, ts, _ = td.decode(ptrs, lengths)
    t_tracked = timed(lambda: td.decode(ptrs, lengths), R)
    t_cf32 = timed(lambda: td.batch.decode_each(outs, lengths, 0.0), R)
    td.close()
    cb = capi.CaptureBatch(ctx, B, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512)
    res8, ts8, _ = cb.decode_estimated(ptrs, lengths)
    t_u8 = timed(lambda: cb.decode_estimated(ptrs, lengths), R)
    cb.close()
    result["tracked_decode"] = dict(seconds=spread(t_tracked), locked=all(r["locked"] == 1 for r in res), ts_packets=[r["ts_packets"] for r in res][:4])
    result["cf32_decode_each_alone"] = dict(seconds=spread(t_cf32))
    result["cu8_decode_estimated"] = dict(seconds=spread(t_u8), ts_packets=[r["ts_packets"] for r in res8][:4],
                                          same_ts_as_tracked=sum(a == b for a, b in zip(ts, ts8)))
    result["tracked_over_cu8_decode_estimated"] = round(statistics.median(t_tracked) / statistics.median(t_u8), 3)
    for b in bufs:
        b.free()

    # ---- a long recording: one tune per piece beside one tune for all
    if args.recording_msamples:
        ns, piece = args.recording_msamples << 20, args.piece_msamples << 20
        overlap = capi.overlap_for(capi.FEC12, bench_c1.OMEGA)
        gen = bench_c1.Generator(capi, ctx, ns, 1)
        cap = gen.capture(0, 7000)[0]
        gen.close()
        P = min(16, len(capi.recording_plan(ns, piece, overlap)))
        rec = {}
        for tune in ("pieces", None):
            dec = capi.RecordingDecoder(ctx, piece, overlap, P, bench_c1.OMEGA, tune=tune)
            ts, report = dec.decode(cap.ptr, ns)
            t = timed(lambda: dec.decode(cap.ptr, ns), R)
            dec.close()
            rec[tune] = (statistics.median(t), ts)
            result["recording_tune_" + str(tune).lower()] = dict(seconds=spread(t), pieces=len(report["pieces"]), pieces_per_batch=P, packets=report["packets"],
                                                                 unjoined=report["unjoined"], tunes=[float(f"{x:.3e}") for x in report["tunes"]][:4])
        result["recording_pieces_minus_none_seconds"] = round(rec["pieces"][0] - rec[None][0], 6)
        result["recording_same_ts"] = bool(rec["pieces"][1] == rec[None][1])
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
