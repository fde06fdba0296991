#!/usr/bin/env python3
"""tools/capture_batch_level.py [--out FILE]

The capture batch's LEVEL CONTRACT, measured: tiles j ≥ 1 start from the constructed AGC (est_insp = 75², gain 1), so the converted,
scaled samples must have an RMS near 75 — how near?  Two true 16-bit captures (synth_dvbs.capture_s16: RMS 75·256; 600 packets seed 11
noise 7.5, and 1500 packets seed 23 noise 18) are decoded as cs16 with in_scale 2^-6 … 2^-10 (RMS 300 … 19) by both engines, and by the
reference binary `oracle/_ref/leandvb --f32 --float-scale <the same value>` on float32(s16).  Per row: the batch's packets, seam_bad,
locked, the reference's packets, and how many of the batch's packets behind the reference's 16th are the reference's, contiguously
(bench_c1.verify's rule).  Writes a table to --out (default profiles/capture_batch_formats/level.txt) and to stdout."""
import argparse
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_c1
import leansdr_amd.capi as capi
from leansdr_amd import synth_dvbs

REFBIN = os.path.join(ROOT, "oracle", "_ref", "leandvb")
CAPTURES = [(600, 11, 7.5), (1500, 23, 18.0)]
EXPONENTS = [-6, -7, -8, -9, -10]


def reference(s16, scale, viterbi):
    args = ["--f32", "--float-scale", repr(scale), "-f", "2400e3", "--sr", "2000e3", "--cr", "1/2"] + (["--viterbi"] if viterbi else [])
    ts = subprocess.run([REFBIN] + args, input=s16.astype(np.float32).tobytes(), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=900).stdout
    return [ts[i:i + 188] for i in range(0, len(ts) // 188 * 188, 188)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_batch_formats", "level.txt"))
    args = ap.parse_args()
    ctx = capi.Ctx(0)
    lines = ["# tools/capture_batch_level.py: cs16 captures of RMS 75*256, anf 1, tile_len 4096; reference = oracle/_ref/leandvb --f32 --float-scale <in_scale>",
             "# capture                      engine   in_scale  rms   batch_packets seam_bad locked  ref_packets  ref_tail_matched/ref_tail  whole_ts_identical"]
    for n_packets, seed, noise in CAPTURES:
        s16, _ = synth_dvbs.capture_s16(n_packets, seed=seed, noise_std=noise)
        n = len(s16) // 2
        buf = ctx.upload(s16)
        jobs = [(e, v) for v in (False, True) for e in EXPONENTS]
        with ThreadPoolExecutor(max_workers=10) as ex:
            refs = list(ex.map(lambda j: reference(s16, 2.0 ** j[0], j[1]), jobs))
        for (e, vit), rpk in zip(jobs, refs):
            scale = 2.0 ** e
            cb = capi.CaptureBatch(ctx, 1, n, bench_c1.OMEGA, anf=1, tile_len=4096, tile_warmup=512, viterbi=True if vit else None,
                                   in_format=capi.IN_CS16, in_scale=scale)
            res, ts = cb.decode([buf.ptr], n)
            cb.close()
            pk = [ts[0][i:i + 188] for i in range(0, len(ts[0]), 188)]
            tail = rpk[bench_c1.SKIP_ACQ:]
            m = 0
            if tail and tail[0] in pk:
                i0 = pk.index(tail[0])
                while m < len(tail) and i0 + m < len(pk) and pk[i0 + m] == tail[m]:
                    m += 1
            r = res[0]
            lines.append(f"{n_packets:5d} packets seed {seed} noise {noise:4.1f}  {'viterbi' if vit else 'default'}  2^{e:<4d}  {75.0 * 256 * scale:6.1f}  "
                         f"{len(pk):6d}        {r['seam_bad']:3d}      {r['locked']}       {len(rpk):6d}       {m:5d}/{len(tail):<5d}               {pk == rpk}")
            print(lines[-1], flush=True)
        buf.free()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
