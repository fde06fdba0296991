"""lsdr_capture_batch at the punctured code rates: both engines at 1/2, 2/3, 3/4, 5/6 and 7/8, samples per symbol held at 6/5.

The captures are made on the CPU by the oracle's leandvbtx | leanchansim (batch_common.rate_capture), not by TxBatch: a fault of the
generator cannot hide one of the decoder.  Behind rate 1/2 deconvol_sync finds the symbol phase of the puncturing pattern only through
next_sync()'s wrap (`locked == 4 → locked = 0, skip = 1`, dvb.h:185-193): up to 15 calls at 7/8, each behind about three search cycles of
mpeg_sync, so a capture loses between 30 and 1600 packets to acquisition and the variants with their first samples dropped walk that path
a different number of times.

  default engine, 2500 packets, nine variants with their own lengths in one decode_each (batch_common.rate_variants):
    a the device-resident tail is the block chain, bit for bit, on the object's own packed decisions: deconvolved bytes, mpeg bytes,
      next_sync() calls, RS counts, lock, TS, and alignment == next_sync_calls % 4;
    b the TS of the seven variants without burst or noise is the reference binary's (`leandvb --cr R --anf 0`) from the first common
      packet on (batch_common.check_from_first_common_packet), the batch at most 192 packets later than the reference;
    c the burst, recorded: what the reference and the batch return behind it (the tail deconvolves everything behind the first lock in
      one call and does not re-acquire a symbol phase; the reference does);
  Viterbi engine, 800 packets, five variants: the bytes are a fresh single-stream lsdr_viterbi_run's at that rate and the rest is
    HostTail's (batch_common._assert_stages_exact), viterbi_sync's bytes stay under symbols // 4, and the TS of the first three is the
    reference binary's under `--viterbi` by batch_common.check_against_reference;
  the workflow of the README once: one front-end pass at FEC12 over a capture of every rate, estimate_fec, group_by_fec, one decoder per
    group, every TS against its reference by rule b.

What b, c and the Viterbi engine measure is printed, and appended to the file LSDR_CAPTURE_RATES_LOG names
(profiles/capture_batch_rates/acquisition.txt).  The reference binary (oracle/_ref/leandvb) is required: where it is missing these tests
FAIL.  Measured on an MI355X: the 26 tests take 12 s, the slowest (7/8, Viterbi engine, with its reference processes) 2.0 s.
"""
import os

import numpy as np
import pytest
from batch_common import (CR, RATE_VARIANTS, _assert_stages_exact, _chain_reference, check_against_reference, check_from_first_common_packet, packets,
                          rate_capture, rate_references, rate_variant, rate_variants, ref_args)

pytestmark = pytest.mark.gpu

RATES = (0, 1, 3, 4, 5)
N_DEFAULT, N_VITERBI = 2500, 800
CLEAN = RATE_VARIANTS[:7]                                  # without burst or noise
BURST, NOISE = RATE_VARIANTS[7], RATE_VARIANTS[8]
VITERBI_VARIANTS = (RATE_VARIANTS[0], RATE_VARIANTS[1], RATE_VARIANTS[4], BURST, NOISE)
DROPPED_2402 = RATE_VARIANTS[5]                            # the variant that acquires fastest at every rate
SYMBOLS_PAST_THE_FILL = 131072                             # (tests/test_gpu_fec_est.py: the generator's interleaver starts from zeros)


LOG_HEADER = """tests/test_gpu_capture_batch_rates.py: lsdr_capture_batch against oracle/_ref/leandvb at the five code rates, 1.2 samples per symbol.
Captures: the oracle's leandvbtx | leanchansim --awgn 17.5 --ou8, 2500 packets (default engine) and 800 (Viterbi engine), anf 0.
late = (reference's packets in front of the first common packet) - (batch's): positive, the batch locked later.  Bound 192.
The reference's own counts at the punctured rates are not the same from run to run (its scheduler follows how its input arrived).
"""


def _log(line):
    print(line)
    path = os.environ.get("LSDR_CAPTURE_RATES_LOG")
    if path:
        new = not os.path.exists(path)
        with open(path, "a") as f:
            if new:
                f.write(LOG_HEADER)
            f.write(line + "\n")


class _Runs:
    """One decode per (engine, rate), made when first asked for and kept — object, buffers, results, TS — until the module is done."""

    def __init__(self, capi, ctx):
        self.capi, self.ctx, self.kept = capi, ctx, {}

    def get(self, rate, viterbi):
        import bench_c1
        key = (rate, viterbi)
        if key not in self.kept:
            capi, ctx = self.capi, self.ctx
            iq = rate_capture(rate, N_VITERBI if viterbi else N_DEFAULT)[0]
            variants = [v for v in rate_variants(iq) if not viterbi or v[0] in VITERBI_VARIANTS]
            bufs = [ctx.upload(v) for _, v in variants]
            cb = capi.CaptureBatch(ctx, len(variants), len(iq) // 2, bench_c1.OMEGA, fec=rate, anf=0, viterbi=True if viterbi else None)
            run = dict(cb=cb, bufs=bufs, names=[v[0] for v in variants])
            try:
                run["res"], run["ts"] = cb.decode_each([b.ptr for b in bufs], [len(v) // 2 for _, v in variants])
            except Exception:
                cb.close()
                for b in bufs:
                    b.free()
                raise
            self.kept[key] = run
        return self.kept[key]

    def close(self):
        for run in self.kept.values():
            run["cb"].close()
            for b in run["bufs"]:
                b.free()
        self.kept = {}


@pytest.fixture(scope="module")
def runs(capi, ctx):
    r = _Runs(capi, ctx)
    yield r
    r.close()


def _references(rate, n_packets, names, *extra):
    return dict(zip(names, rate_references([(rate, n_packets, name, ref_args(rate, *extra, "--anf", "0")) for name in names])))


# ---- a -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_device_resident_tail_equals_the_block_chain_at_every_rate(capi, ctx, runs, rate):
    run = runs.get(rate, False)
    cb, res, ts, names = run["cb"], run["res"], run["ts"], run["names"]
    assert tuple(names) == RATE_VARIANTS
    for i, name in enumerate(names):
        r = res[i]
        words_dev = capi.lib.lsdr_capture_batch_words_dev(cb.h, i)
        byte_cap = r["symbols"] // 4 + 65536                     # (under two bits per symbol at any rate: never in the way)
        want_bytes, want_mpeg, want_ts, st = _chain_reference(capi, ctx, words_dev, r["symbols"], byte_cap, cb.unlocked_window, rate=rate)
        got_bytes = cb.stage_bytes(i, "deconv", r["bytes_deconv"])
        got_mpeg = cb.stage_bytes(i, "mpeg", r["bytes_mpeg"])
        print(f"rate {CR[rate]}, {name}: {r}")
        assert r["bytes_deconv"] == len(want_bytes) and got_bytes.tobytes() == want_bytes.tobytes(), name
        assert r["bytes_mpeg"] == len(want_mpeg) and got_mpeg.tobytes() == want_mpeg.tobytes(), name
        assert r["next_sync_calls"] == st["next_sync"] and r["rs_packets"] == st["npk"] and r["locked"] == st["locked"], (name, r, st)
        assert r["rs_bit_errors"] == st["errs"], (name, r, st)
        assert ts[i] == want_ts.tobytes(), name
        assert r["alignment"] == r["next_sync_calls"] % 4, (name, r)
    # conditions on the inputs (they hold for the reference binary: measured on the CPU)
    by = dict(zip(names, res))
    if rate != capi.FEC12:
        calls = [r["next_sync_calls"] for r in res]
        assert len(set(calls)) >= 3, calls                                                       # the variants walk the skip path differently
        assert any(r["next_sync_calls"] >= 4 and r["ts_packets"] > 700 for r in res), res         # … through the wrap, and decoded behind it
    assert by[NOISE]["locked"] == 0 and by[NOISE]["ts_packets"] == 0 and by[NOISE]["next_sync_calls"] >= 8, by[NOISE]
    assert 200 < by[BURST]["ts_packets"] < by[RATE_VARIANTS[0]]["ts_packets"], (by[BURST], by[RATE_VARIANTS[0]])


# ---- b -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_ts_is_the_reference_binarys_at_every_rate(runs, rate):
    sent = rate_capture(rate, N_DEFAULT)[1]
    refs = _references(rate, N_DEFAULT, CLEAN)
    run = runs.get(rate, False)
    failures = []
    for name, r, ts in zip(run["names"], run["res"], run["ts"]):
        if name not in CLEAN:
            continue
        what = f"default engine, rate {CR[rate]}, {name}"
        try:
            c = check_from_first_common_packet(ts, refs[name], sent, what)
            _log(f"{what}: late {c['late']}, batch {c['batch']} packets, reference {c['reference']}, compared {c['compared']}, "
                 f"next_sync_calls {r['next_sync_calls']}")
        except AssertionError as e:                               # (every variant is measured before the first failure is raised)
            _log(f"{what}: FAILED {e}; batch {len(ts) // 188} packets, reference {len(refs[name]) // 188}, next_sync_calls {r['next_sync_calls']}")
            failures.append(e)
    if failures:
        raise failures[0]


# ---- c -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_burst_is_recorded_at_every_rate(runs, rate):
    """Recorded, not asserted equal: behind the burst the reference changes alignment and symbol phase and relocks, the tail has
    deconvolved everything behind its first lock with the alignment and phase it had there."""
    ref = _references(rate, N_DEFAULT, (BURST,))[BURST]
    run = runs.get(rate, False)
    i = run["names"].index(BURST)
    got, r = run["ts"][i], run["res"][i]
    assert len(ref) % 188 == 0 and len(got) % 188 == 0
    rset = set(packets(ref))
    common = sum(p in rset for p in packets(got))
    _log(f"default engine, rate {CR[rate]}, {BURST}: batch {len(got) // 188} packets, reference {len(ref) // 188}, in both {common}, "
         f"next_sync_calls {r['next_sync_calls']}, locked at the end {r['locked']}")


# ---- the Viterbi engine ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_viterbi_stage_and_tail_are_exact_at_every_rate(capi, ctx, runs, rate):
    run = runs.get(rate, True)
    cb, res, ts, names = run["cb"], run["res"], run["ts"], run["names"]
    assert tuple(names) == VITERBI_VARIANTS
    _assert_stages_exact(capi, ctx, cb, res, ts, names, rate)
    for name, r in zip(names, res):
        assert r["bytes_deconv"] <= r["symbols"] // 4, (name, r)                                  # the tail's byte buffers hold soft_cap / 4 + 64
    by = dict(zip(names, res))
    assert by[NOISE]["ts_packets"] == 0 and by[NOISE]["locked"] == 0, by[NOISE]
    assert 200 < by[BURST]["ts_packets"] < by[names[0]]["ts_packets"], (by[BURST], by[names[0]])


@pytest.mark.parametrize("rate", RATES)
def test_viterbi_ts_is_the_reference_binarys_at_every_rate(runs, rate):
    sent = rate_capture(rate, N_VITERBI)[1]
    refs = _references(rate, N_VITERBI, VITERBI_VARIANTS[:4], "--viterbi")
    run = runs.get(rate, True)
    cb = run["cb"]
    for i, name in enumerate(run["names"]):
        st = cb.viterbi_stats(i)
        line = f"viterbi engine, rate {CR[rate]}, {name}: batch {len(run['ts'][i]) // 188} packets"
        if name in refs:
            line += f", reference {len(refs[name]) // 188}"
        _log(line + f", rounds {st['rounds']}, batch rounds {st['batch_rounds']}, switches {st['switches']}")
    import bench_c1
    for i, name in enumerate(run["names"][:3]):
        # Behind leandvbtx the reference's own first packets (two to four, measured) come out of the deinterleaver's fill and were never
        # transmitted.  Condition on the input: they are few, and all in front of the first compared packet; the batch may return those
        # and no other packet that was not transmitted.
        rpk = packets(refs[name])
        fill = {p for p in rpk if p not in sent}
        assert len(fill) <= 8 and fill <= set(rpk[:bench_c1.SKIP_ACQ]), f"{name}: invalid input, {len(fill)} of the reference's packets were never transmitted"
        check_against_reference(run["ts"][i], refs[name], sent | fill, 700, f"viterbi engine, rate {CR[rate]}, {name}", False)


# ---- the workflow ------------------------------------------------------------------------------------------------------------------
def test_estimate_group_and_decode_a_job_of_every_rate(capi, ctx):
    import bench_c1
    iqs = [rate_variant(r, N_DEFAULT, DROPPED_2402) for r in RATES]
    lengths = [len(iq) // 2 for iq in iqs]
    n = max(lengths)
    padded = [np.concatenate([iq, iq[: 2 * n - len(iq)]]) for iq in iqs]                          # each repeated from its own start
    bufs = [ctx.upload(p) for p in padded]
    try:
        front = capi.CaptureBatch(ctx, len(RATES), n, bench_c1.OMEGA, fec=capi.FEC12, anf=0)
        try:
            front.run_async([b.ptr for b in bufs], n)
            res = front.wait()
            est = front.estimate_fec(res, max_symbols=SYMBOLS_PAST_THE_FILL)
        finally:
            front.close()
        for r, e in zip(RATES, est):
            print(f"transmitted {CR[r]}: {e}")
        groups, left = capi.group_by_fec(est)
        assert groups == [(r, [i]) for i, r in enumerate(RATES)] and left == [], (groups, left)
        refs = rate_references([(r, N_DEFAULT, DROPPED_2402, ref_args(r, "--anf", "0")) for r in RATES])
        for fec, members in groups:
            (i,) = members
            cb = capi.CaptureBatch(ctx, 1, lengths[i], bench_c1.OMEGA, fec=fec, anf=0)
            try:
                _, ts = cb.decode([bufs[i].ptr], lengths[i])                                      # (the capture itself, without its padding)
            finally:
                cb.close()
            check_from_first_common_packet(ts[0], refs[i], rate_capture(RATES[i], N_DEFAULT)[1], f"workflow, rate {CR[fec]}")
    finally:
        for b in bufs:
            b.free()
