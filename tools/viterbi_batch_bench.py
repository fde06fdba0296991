#!/usr/bin/env python3
"""tools/viterbi_batch_bench.py [--once] [--out FILE] — B device-resident locked QPSK 1/2 streams decoded (a) by one ViterbiBatch and
(b) by B lsdr_viterbi_run streams one after the other on the same context, in one process, the two ways alternating after a warm-up
of both.  B = 1, 8, 32; 1 Mi and 16 Mi symbols per stream (below and above the length at which one stream alone fills the chip).

The streams are fec_input of the tiled golden symbols at 40 per mille, as in the tests.  The first pass of both ways starts from fresh
decoders and its bytes are compared, every stream of (a) against (b); the timed passes decode the same buffers again with the carried
states (a locked stream goes on).  A pass = every stream's whole input, however many runs / calls that takes; times are host clocks
around work that ends in wait / in the synchronous call.  Writes one JSON line (per length and B: seconds per pass of each way, their
ratio b / a, the spread (max − min) / median over the repeats, launches per run, runs per stream) to profiles/viterbi_batch/bench.json.
Exit status 1 when the batch at B = 32 is slower than (b) by more than (b)'s own spread.
--once: one small case (B = 8, 1 Mi symbols), one pass of each way after the warm-up — for a kernel trace."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import leansdr_amd.capi as capi
from fec_common import fec_input, hard_symbols


def make_stream(n):
    hard = hard_symbols()
    return fec_input(np.tile(hard, (n + len(hard) - 1) // len(hard))[:n], 40)


class Case:
    def __init__(self, ctx, sym, B):
        self.ctx, self.B, self.n = ctx, B, len(sym)
        self.total = len(sym) // 128 * 128
        first = ctx.upload(sym)
        self.ins = [first]
        for _ in range(B - 1):                       # B copies of their own: no stream rides on another's cache lines
            d = ctx.alloc(sym.nbytes)
            capi.check(capi.lib.lsdr_memcpy_d2d(ctx.h, d.ptr, first.ptr, sym.nbytes))
            self.ins.append(d)
        ctx.sync()
        self.cap = len(sym) // 8 + 64
        self.out_a = [ctx.alloc(self.cap) for _ in range(B)]
        self.out_b = [ctx.alloc(self.cap) for _ in range(B)]
        self.vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, B, len(sym))
        self.vs = [capi.Viterbi(ctx, capi.QPSK, capi.FEC12) for _ in range(B)]
        self.launches, self.runs_a, self.calls_b = 0, 0, 0

    def pass_a(self):
        pos, nout, runs = [0] * self.B, [0] * self.B, 0
        while any(p < self.total for p in pos):
            self.vb.run_async_dev([d.at(4 * p) for d, p in zip(self.ins, pos)], [self.n - p for p in pos],
                                  [d.at(o) for d, o in zip(self.out_a, nout)], self.cap - max(nout))
            res = self.vb.wait()
            runs += 1
            if runs == 1:
                self.launches = self.vb.stats()["launches_last_run"]
            for i, r in enumerate(res):
                pos[i] += r["consumed"]
                nout[i] += r["produced"]
            assert any(r["consumed"] for r in res), "no progress"
        self.runs_a = runs
        return nout

    def pass_b(self):
        calls, nouts = 0, []
        for v, din, dout in zip(self.vs, self.ins, self.out_b):
            pos = nout = 0
            while pos < self.total:
                c, p = v.run_dev(din.at(4 * pos), self.n - pos, dout.at(nout), self.cap - nout)
                calls += 1
                assert c, "no progress"
                pos += c
                nout += p
            nouts.append(nout)
        self.calls_b = calls
        return nouts

    def compare(self, na, nb):
        assert na == nb, (na, nb)
        for i in range(self.B):
            a = self.ctx.download(self.out_a[i], np.uint8, na[i])
            b = self.ctx.download(self.out_b[i], np.uint8, nb[i])
            assert a.tobytes() == b.tobytes(), f"stream {i}: the batch's bytes differ from lsdr_viterbi_run's"

    def close(self):
        self.vb.close()
        for v in self.vs:
            v.close()
        for d in self.ins + self.out_a + self.out_b:
            d.free()


def timed(fn, min_seconds):
    t0 = time.perf_counter()
    k = 0
    while True:
        fn()
        k += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / k


def stats(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2]
    return med, (xs[-1] - xs[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viterbi_batch", "bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    ctx = capi.Ctx(0)
    if args.once:
        c = Case(ctx, make_stream(1 << 20), 8)
        c.compare(c.pass_a(), c.pass_b())            # warm-up of both, from fresh decoders, bytes compared
        c.pass_a()
        c.pass_b()
        print(json.dumps(dict(once=True, B=8, symbols=1 << 20, launches_per_run=c.launches, runs_a=c.runs_a, calls_b=c.calls_b)))
        c.close()
        ctx.close()
        return 0
    rows, ok = [], True
    for n in (1 << 20, 16 << 20):
        sym = make_stream(n)
        for B in (1, 8, 32):
            c = Case(ctx, sym, B)
            c.compare(c.pass_a(), c.pass_b())
            runs_first, calls_first = c.runs_a, c.calls_b
            ta, tb = [], []
            for _ in range(args.repeats):
                ta.append(timed(c.pass_a, 0.2))
                tb.append(timed(c.pass_b, 0.2))
            a, sa = stats(ta)
            b, sb = stats(tb)
            row = dict(symbols=n, B=B, batch_s=a, loop_s=b, ratio_loop_over_batch=b / a, spread_batch=sa, spread_loop=sb,
                       batch_gsym_s=B * c.total / a / 1e9, loop_gsym_s=B * c.total / b / 1e9, launches_per_run=c.launches,
                       runs_per_stream_first_pass=runs_first, runs_per_stream=c.runs_a, loop_calls_per_stream=c.calls_b / B,
                       loop_calls_per_stream_first_pass=calls_first / B)
            if B == 32:
                row["accepted"] = bool(a <= b * (1 + sb))
                ok = ok and row["accepted"]
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
            c.close()
    line = json.dumps(dict(tool="viterbi_batch_bench", repeats=args.repeats, accepted=ok, cases=rows))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
