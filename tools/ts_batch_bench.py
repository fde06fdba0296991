#!/usr/bin/env python3
"""tools/ts_batch_bench.py [--streams 32] [--packets 68489] [--repeats 7] [--msamples 8] [--out FILE]

What the census and the PID filter of many transport streams (lsdr_ts_batch) cost, one GPU.  The input: `streams` streams of `packets`
packets (what one 128 Mi sample capture of the c1 job decodes to: 412 MB of TS per step at 32 captures) built on the host — 12 PIDs with correct continuity counters, 30 % null
packets, one PID with 58 % of the rest — and uploaded.  After one warm-up each, `repeats` times on the host clock, in one process:

  * the census alone, lsdr_ts_batch_run_async → lsdr_ts_batch_wait (the C calls; once more through capi.TsBatch.census, which also
    builds the Python dictionaries), at every tile size (LSDR_TS_BATCH_TILE, read at create); beside it the bytes of the packet
    headers it needs (8 per packet) and the 64-byte pieces of memory they lie in, each over 8 TB/s — the memory-side floor;
  * census plus filter, run_async → wait: every packet kept, null packets dropped, one PID of 12 kept;
  * the download of what each of these three rules kept into pinned host memory, download_async → download_wait: "every packet" is the
    full copy lsdr_capture_batch_ts_download_async makes of the same bytes.  Checked: a download moves kept·188 bytes per stream;
  * for scale, at the bench condition (bench_c1.Generator: QPSK 1/2, 1.2 samples per symbol, cu8): the default-engine capture batch
    (anf 1, tile_len 4096) decoding `streams` captures of `msamples` Mi samples, and ts_census on the TS that decode left on the device.

Nothing is a threshold.  The decode kernels are the parent commit's.

Writes one JSON line to --out (default profiles/ts_batch/bench.json) and to stdout."""
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
PIDS = [0x000, 0x011, 0x100, 0x101, 0x102, 0x110, 0x111, 0x120, 0x121, 0x130, 0x131, 0x1fff]      # 11 and the null PID
SHARE = [0.005, 0.005, 0.406, 0.06, 0.04, 0.05, 0.03, 0.04, 0.02, 0.03, 0.014, 0.30]


def spread(ts):
    return dict(median=round(statistics.median(ts), 6), min=round(min(ts), 6), max=round(max(ts), 6), n=len(ts))


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def build(n, seed):
    """n packets on the 12 PIDs, every PID's counter stepping by one per packet (all carry payload)."""
    rng = np.random.default_rng(seed)
    which = rng.choice(len(PIDS), n, p=SHARE)
    pk = rng.integers(0, 256, (n, 188)).astype(np.uint8)
    pid = np.asarray(PIDS)[which]
    cc = np.zeros(n, np.int64)
    for k in range(len(PIDS)):
        at = np.flatnonzero(which == k)
        cc[at] = np.arange(len(at)) & 15
    pk[:, 0], pk[:, 1], pk[:, 2], pk[:, 3] = 0x47, pid >> 8, pid & 255, 0x10 | cc
    return pk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--packets", type=int, default=68489)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--msamples", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ts_batch", "bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench_c1
    import leansdr_amd.capi as capi
    B, n = args.streams, args.packets
    ctx = capi.Ctx(0)
    result = dict(tool="tools/ts_batch_bench.py", repeats=args.repeats, streams=B, packets=n, ts_bytes=B * n * 188)
    bufs = [ctx.upload(build(n, 100 + i)) for i in range(B)]
    ptrs, lengths = [b.ptr for b in bufs], [n] * B

    census = {}
    for tile in (256, 512, 768, 1024):
        os.environ["LSDR_TS_BATCH_TILE"] = str(tile)
        tb = capi.TsBatch(ctx, B, n)
        del os.environ["LSDR_TS_BATCH_TILE"]
        got = tb.census(ptrs, lengths)                                          # warm-up

        def run():                                                              # the C calls alone: no dictionaries are built
            tb.run_async(ptrs, lengths)
            capi.check(capi.lib.lsdr_ts_batch_wait(tb.h, tb._sum))
        census[str(tb.tile)] = spread(timed(run, args.repeats))
        if tile == 1024:
            result["census_with_python_dicts_seconds"] = spread(timed(lambda: tb.census(ptrs, lengths), args.repeats))
        tb.close()
    assert all(s["cc_errors"] == 0 and s["pids_seen"] == len(PIDS) and s["valid"] == n for s in got), got[0]
    result["census_seconds_by_tile"] = census
    result["census_header_bytes"] = B * n * 8
    result["census_header_bytes_over_8TBps_seconds"] = float(f"{B * n * 8 / HBM_BYTES_PER_S:.3e}")
    result["census_64_byte_pieces_over_8TBps_seconds"] = float(f"{B * n * 64 / HBM_BYTES_PER_S:.3e}")
    result["null_share"] = round(got[0]["null_packets"] / n, 4)

    tb = capi.TsBatch(ctx, B, n)
    result["tile"] = tb.tile
    host = []
    for _ in range(B):
        p = C.c_void_p()
        capi.check(capi.lib.lsdr_malloc_host(n * 188, C.byref(p)))
        host.append(p)
    hp = (C.c_void_p * B)(*host)
    for name, kw in (("every_packet", dict(keep_pids=None, drop_null=False, drop_tei=False, drop_sync=False)),
                     ("drop_null", dict(keep_pids=None)), ("one_pid_of_12", dict(keep_pids=[0x101]))):
        rule, keep = tb.rule(**kw)

        def run():
            tb.run_async(ptrs, lengths, rule)
            capi.check(capi.lib.lsdr_ts_batch_wait(tb.h, tb._sum))
            return tb._sum

        def download():
            capi.check(capi.lib.lsdr_ts_batch_download_async(tb.h, hp, n * 188))
            tb.download_wait()
        res = run()                                                             # warm-up
        t_run = timed(run, args.repeats)
        download()
        t_dl = timed(download, args.repeats)
        res = [dict(kept=int(s.kept)) for s in res[:B]]
        kept = sum(s["kept"] for s in res)
        # the only condition: a filtered download moves kept·188 bytes per stream (the first and the last kept packet arrived)
        for i in (0, B - 1):
            a = np.ctypeslib.as_array(C.cast(host[i], C.POINTER(C.c_uint8)), (n * 188,))
            k = res[i]["kept"]
            want = np.empty(k * 188, np.uint8)
            capi.check(capi.lib.lsdr_memcpy_d2h(ctx.h, want.ctypes.data, tb.out_ptr(i), want.nbytes))
            ctx.sync()
            assert np.array_equal(a[:k * 188], want), (name, i)
        result[name] = dict(kept_packets=kept, kept_bytes=kept * 188, census_and_filter_seconds=spread(t_run), download_seconds=spread(t_dl),
                            download_GBps=round(kept * 188 / statistics.median(t_dl) / 1e9, 2))
    tb.close()
    for p in host:
        capi.check(capi.lib.lsdr_free_host(p))
    for b in bufs:
        b.free()

    ns = args.msamples << 20
    gen = bench_c1.Generator(capi, ctx, ns, B)
    caps = [gen.capture(k, 7000 + k)[0] for k in range(B)]
    gen.close()
    cptrs = [b.ptr for b in caps]
    cb = capi.CaptureBatch(ctx, B, ns, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512)

    def decode():
        cb.run_async(cptrs, ns)
        return cb.wait()
    res = decode()                                                              # warm-up
    t_dec = timed(decode, args.repeats)
    got = cb.ts_census(res)                                                     # warm-up
    tsb, tptrs, tn = cb._ts_object(res)

    def census_c():
        tsb.run_async(tptrs, tn)
        capi.check(capi.lib.lsdr_ts_batch_wait(tsb.h, tsb._sum))
    t_cen = timed(census_c, args.repeats)
    result["decode"] = dict(workload=f"B = {B} x {args.msamples} Mi samples cu8, QPSK 1/2 at 1.2 samples per symbol; default engine, anf 1, tile_len 4096",
                            seconds=spread(t_dec), ts_packets=[r["ts_packets"] for r in res][:4])
    result["ts_census_after_decode"] = dict(seconds=spread(t_cen), pids_seen=got[0]["pids_seen"], cc_errors=[s["cc_errors"] for s in got][:4],
                                            cc_missing=[s["cc_missing"] for s in got][:4])
    result["ts_census_over_decode"] = round(statistics.median(t_cen) / statistics.median(t_dec), 5)
    cb.close()
    for b in caps:
        b.free()
    ctx.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
