"""The inputs of the re-acquisition tests, pinned on the CPU: relock_common.chain_cpu — the loop that defines the feature, on the oracle's
deconvol_sync and mpeg_sync — over the decisions of the oracle's serial cstln_receiver.

  · the table the feature was specified with: rate 1/2, 1200 packets, a burst of n/40 samples at n/2 — 549 TS packets under today's
    schedule, 927 with windows all the way (1 next_sync, ends locked); with a step of 180 degrees behind the burst 549 → 911; two
    steps (180 at n/3, 270 at 2n/3): 664 / 571 / 727 packets at relocks 0 / 1 / 2 and more; three steps (90, 180, 270 at n/4, n/2, 3n/4):
    486 / 566 / 566 / 599 at 0 / 1 / 2 / 3 and more.  A capped run is not always at least as good as today's: 571 < 664;
  · relocks = 0 is batch_common._chain_reference's rule (the whole remainder as soon as mpeg_sync is locked), byte for byte;
  · every capture the GPU tests use returns, from packet bench_c1.SKIP_ACQ on, packets that were transmitted — by
    relock_common.assert_transmitted, which has one exception and says why: behind a re-acquisition the derandomizer passes up to
    seven packets before it meets an inverted sync byte.  "All of them" holds for no capture that re-acquires (6 such packets behind the
    burst of the 549 → 927 capture), so the captures stay the specified ones and the rule names the exception.
No GPU.
"""
import functools

import pytest
import relock_common as rc
from batch_common import rate_capture

WINDOW = 8192


@functools.lru_cache(maxsize=None)
def _symbols(rate, n_packets, name):
    iq = rate_capture(rate, n_packets)[0]
    if name == "step 180 deg" and n_packets != 1200:
        return rc.oracle_symbols(rc.single_step(iq, 180))
    return rc.oracle_symbols(dict(rc.relock_batch(rate, n_packets))[name])


def _packets(oracle, name, relocks, rate=0, n_packets=1200):
    return rc.chain_cpu(oracle, _symbols(rate, n_packets, name), rate, WINDOW, relocks)


def test_the_specified_table(oracle):
    today, windows = _packets(oracle, "step 0 deg", 0), _packets(oracle, "step 0 deg", 16)
    assert (len(today["ts"]), today["locked"]) == (549, 0) and (len(windows["ts"]), windows["locked"], windows["next_sync"]) == (927, 1, 1)
    assert len(today["bytes"]) == 242521 and len(windows["bytes"]) == 242517       # the windowed schedule ends a few bytes short of the one call
    assert [len(_packets(oracle, "step 180 deg", r)["ts"]) for r in (0, 16)] == [549, 911]
    two = [_packets(oracle, "two steps", r) for r in (0, 1, 2, 3, 16)]
    assert [len(t["ts"]) for t in two] == [664, 571, 727, 727, 727]
    assert (two[2]["locks"], two[2]["next_sync"]) == (3, 2)
    three = [_packets(oracle, "three steps", r) for r in (0, 1, 2, 3, 16)]
    assert [len(t["ts"]) for t in three] == [486, 566, 566, 599, 599] and three[3]["locks"] == 4


@pytest.mark.parametrize("name", ["clean", "step 90 deg", "two steps", "noise only"])
def test_relocks_0_is_todays_schedule(oracle, name):
    sym = _symbols(0, 1200, name)
    a = rc.chain_cpu(oracle, sym, 0, WINDOW, 0)
    b = rc.chain_cpu(oracle, sym, 0, WINDOW, None, bulk_rule=lambda locked, locks: locked)      # _chain_reference: `if t.msync.locked`
    assert a["ts"] == b["ts"] and a["bytes"].tobytes() == b["bytes"].tobytes() and a["mpeg"].tobytes() == b["mpeg"].tobytes()
    assert (a["locked"], a["locks"], a["next_sync"]) == (b["locked"], b["locks"], b["next_sync"])


def _sent(rate, n_packets):
    from leansdr_amd import synth_dvbs
    return [bytes(p) for p in synth_dvbs.ts_packets(n_packets, start=1000 * rate)]


@pytest.mark.parametrize("relocks", [0, 1, 3])
def test_the_gpu_tests_captures_return_transmitted_packets(oracle, relocks):
    sent = _sent(0, 1200)
    assert set(sent) == rate_capture(0, 1200)[1]
    for name, _ in rc.relock_batch(0, 1200):
        out = _packets(oracle, name, relocks)
        runs = rc.assert_transmitted(out["ts"], sent, out["locks"], f"{name}, relocks {relocks}")
        print(f"{name}, relocks {relocks}: {len(out['ts'])} packets, {out['locks']} locks, runs behind re-acquisitions {runs}")


@pytest.mark.parametrize("rate", [3, 5])
def test_the_punctured_captures_return_transmitted_packets(oracle, rate):
    out = _packets(oracle, "step 180 deg", 3, rate, 2500)
    runs = rc.assert_transmitted(out["ts"], _sent(rate, 2500), out["locks"], f"rate {rate}")
    print(f"rate {rate}: {len(out['ts'])} packets, {out['locks']} locks, {out['next_sync']} next_sync, runs {runs}")
    assert len(out["ts"]) >= 500
