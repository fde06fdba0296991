"""lsdr_ts_batch's definition without a GPU: the numpy restatement (ts_common.census) against answers derivable by hand — what the device
is then held to bit for bit in test_gpu_ts_batch.py.

leantsgen's pattern (synth_dvbs.ts_packets): byte 0 = 0x47, bytes 1 … 3 the 24-bit packet counter t.  So pid = (t >> 8) & 0x1fff,
cc = t & 15, afc = (t >> 4) & 3.  The counter steps with every packet, but only a packet with payload (afc odd) may step it: of the 256
packets of one PID the 128 with afc even are errors, each missing 1, and the PID's first packet is not judged — 127 errors per complete
PID.  Byte 4 is 4 and byte 5 is t >> 16 (0 or 1): no discontinuity flag, no PCR.
"""
import numpy as np
import ts_common as tc
from leansdr_amd import synth_dvbs


def test_leantsgen_256_packets_one_pid():
    s = tc.census(synth_dvbs.ts_packets(256))
    assert s["packets"] == s["valid"] == 256 and s["pids_seen"] == 1 and s["sync_errors"] == s["tei"] == s["null_packets"] == 0
    assert s["cc_errors"] == 127 and s["cc_missing"] == 127 and s["cc_repeats"] == 0 and s["discontinuities"] == 0
    assert s["pcr_pid"] == -1 and s["pcr_count"] == 0
    p, = s["pids"]
    assert p == dict(pid=0, packets=256, pusi=0, scrambled=192, cc_errors=127, cc_repeats=0, cc_missing=127, discontinuities=0, pcr_count=0,
                     first_packet=0, last_packet=255)                     # scrambled: t & 0xc0 != 0 for t >= 64


def test_leantsgen_4096_packets_16_pids():
    s = tc.census(synth_dvbs.ts_packets(4096))
    assert s["pids_seen"] == s["pids_listed"] == 16 and s["cc_errors"] == 2032 and s["cc_missing"] == 2032
    assert [p["pid"] for p in s["pids"]] == list(range(16)) and all(p["packets"] == 256 and p["cc_errors"] == 127 for p in s["pids"])
    assert [(p["first_packet"], p["last_packet"]) for p in s["pids"]] == [(256 * i, 256 * i + 255) for i in range(16)]


def test_leantsgen_70000_packets_more_pids_than_the_default_table():
    ts = synth_dvbs.ts_packets(70000)
    s = tc.census(ts)
    assert s["pids_seen"] == 274 and s["pids_listed"] == 64 and [p["pid"] for p in s["pids"]] == list(range(64))
    # 273 complete PIDs and one of 70000 − 273·256 = 112 packets: t = 69888 … 69999, afc even for the first 16 of every 32: 64, none unjudged but the first
    assert s["cc_errors"] == 273 * 127 + 63 == s["cc_missing"]
    full = tc.census(ts, 8192)
    assert full["pids_listed"] == 274 and [p["pid"] for p in full["pids"]] == list(range(274)) and full["pids"][-1]["packets"] == 112
    assert {k: v for k, v in full.items() if k not in ("pids", "pids_listed")} == {k: v for k, v in s.items() if k not in ("pids", "pids_listed")}


def test_the_builders_stream_gives_exactly_its_injected_events(capi):
    for n in (3000, 600):
        ts, want = tc.build_stream(n)
        s = tc.census(ts)
        assert len(ts) == n + 3 - 5 == want["packets"] == s["packets"]
        for k in ("sync_errors", "tei", "cc_errors", "cc_missing", "cc_repeats", "discontinuities", "pcr_pid"):
            assert s[k] == want[k], (n, k, s[k], want[k])
        assert s["pids_seen"] == 5 and [p["pid"] for p in s["pids"]] == [tc.PAT, tc.VIDEO, tc.AUDIO, tc.DATA, tc.NULL_PID]
        for p in s["pids"]:
            assert {k: p[k] for k in want["per_pid"][p["pid"]]} == want["per_pid"][p["pid"]], (n, p)
        assert s["valid"] == s["packets"] - 4 and s["null_packets"] == s["pids"][-1]["packets"] > n // 10
        assert sum(p["packets"] for p in s["pids"]) == s["valid"]
        # the PCRs: on video only, the base wraps between the first and the last, and the bit rate is the builder's
        video = s["pids"][1]
        assert s["pcr_count"] == video["pcr_count"] >= 4 and s["pcr_last"] < s["pcr_first"] and s["pcr_first_packet"] == video["first_packet"]
        assert capi.ts_bitrate(s) == 188 * 8 * 27e6 / tc.TICKS_PER_PACKET
        assert any(p["scrambled"] for p in s["pids"]) and video["pusi"] > 0


def test_the_selection_of_a_rule():
    ts, _ = tc.build_stream(600)
    f = tc.fields(ts)
    everything = tc.kept(ts, None, False, False, False)
    assert list(everything) == list(range(len(ts)))
    default = tc.kept(ts)
    assert len(default) == len(ts) - 4 - int(((f["cls"] == 0) & (f["pid"] == tc.NULL_PID)).sum())
    audio = tc.kept(ts, [tc.AUDIO])
    assert len(audio) and all(f["pid"][audio] == tc.AUDIO) and all(f["cls"][audio] == 0)
    with_bad = tc.kept(ts, [tc.AUDIO], drop_tei=False, drop_sync=False)
    assert len(with_bad) == len(audio) + 4                                  # sync-error and TEI packets have no PID: the list does not apply
    assert len(tc.kept(ts, [])) == 0
    assert np.array_equal(np.frombuffer(tc.select(ts, everything), np.uint8), ts.reshape(-1))
