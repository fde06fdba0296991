"""capi.RecordingDecoder: one capture decoded in overlapping pieces whose transport streams are joined on the device (lsdr_ts_stitch).

The capture is batch_common.capture(2500, 3, 7.5) — 4 896 023 cu8 samples at 1.2 samples per symbol, rate 1/2 — in pieces of 1 000 000
samples that overlap by 500 000: nine pieces.  The references are the reference binary (oracle/_ref/leandvb, required: its callers fail
where it is missing) on the whole capture and on every piece, and the numpy restatement of the stitch (stitch_common).

  (a) decode's TS is the restatement's stitch of the device's own per-piece TS, byte for byte: default engine in one batch, default engine
      four pieces at a time (two joins cross a batch boundary), the Viterbi engine at noise 18, the --hs graph
  (b) every join has joined = 1
  (c) no packet stands twice: the 24-bit counter in bytes 1 … 3, from the first derandomised packet on
  (d) from the first packet both have, the stitched TS is the reference's whole-capture TS packet for packet; at most the whole TS's last
      8 packets (one derandomiser group) are not reached, and the stitched TS has nothing behind them.  The bound is a condition: the
      reference's own pieces, stitched by the restatement, lose exactly 1 packet on this capture
  (e) decode_file on the same samples in a file returns decode's bytes
  (f) with the middle piece replaced by noise the two joins of that piece are reported unjoined, every other pair joins, no packet that a
      piece produced is lost and none stands twice.  The piece behind the noise acquires 8 packets later than its right neighbour, which
      starts in the clear: the stitch's definition alone drops those 8 with the neighbour's head (measured: 8 packets of piece 6 lost);
      the decoder takes the neighbour's packets in front of the run there (report["pieces"][k]["head_in_front"], "dropped_in_front")
"""
from concurrent.futures import ThreadPoolExecutor

import batch_common as bc
import numpy as np
import pytest
import stitch_common as sc

pytestmark = pytest.mark.gpu

PIECE, OVERLAP, WINDOW, MIN_RUN = 1000000, 500000, 4096, 8
CONFIGS = {"default": dict(noise=7.5, args=bc.REF_U8, kw=dict(pieces_per_batch=9)),
           "default, 4 per batch": dict(noise=7.5, args=bc.REF_U8, kw=dict(pieces_per_batch=4)),
           "viterbi": dict(noise=18.0, args=bc.REF_U8 + ("--viterbi",), kw=dict(pieces_per_batch=9, viterbi=True)),
           "hs": dict(noise=7.5, args=bc.REF_U8 + ("--hs",), kw=dict(pieces_per_batch=9, hs=True))}


def decode(capi, ctx, iq, **kw):
    """(TS, report) of the capture `iq` through a RecordingDecoder that keeps every piece's TS."""
    buf = ctx.upload(iq)
    dec = capi.RecordingDecoder(ctx, PIECE, OVERLAP, omega=1.2, window=WINDOW, min_run=MIN_RUN, piece_ts=True, **kw)
    try:
        return dec.decode(buf.ptr, len(iq) // 2)
    finally:
        dec.close()
        buf.free()


@pytest.fixture(scope="module")
def runs(capi, ctx):
    """decode of every configuration, once."""
    return {name: decode(capi, ctx, bc.capture(2500, 3, c["noise"])[0], **c["kw"]) for name, c in CONFIGS.items()}


def counters(ts, sent):
    """The 24-bit counters of the TS's packets from the first transmitted (derandomised) one on."""
    pk = bc.packets(ts)
    first = next(i for i, p in enumerate(pk) if p in sent)
    return [(p[1] << 16) | (p[2] << 8) | p[3] for p in pk[first:]]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_decode_is_the_stitch_of_its_pieces(capi, runs, name):
    ts, report = runs[name]
    sent = bc.capture(2500, 3, CONFIGS[name]["noise"])[1]
    assert len(report["pieces"]) == 9 == len(capi.recording_plan(4896023, PIECE, OVERLAP)) and len(report["joins"]) == 8
    joins, keep, want = sc.stitch([p["ts"] for p in report["pieces"]], WINDOW, MIN_RUN)                  # (a)
    print(name, "tune", report["tune"], "packets", report["packets"], [j["run"] for j in report["joins"]], [p["keep"] for p in report["pieces"]])
    assert report["joins"] == joins and [p["keep"] for p in report["pieces"]] == [[k["start"], k["end"]] for k in keep]
    assert ts == want and report["packets"] * 188 == len(ts)
    assert all(j["joined"] == 1 for j in report["joins"]) and report["unjoined"] == []                   # (b)
    c = counters(ts, sent)
    assert len(set(c)) == len(c) and c == sorted(c) and len(c) > 2300                                    # (c)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_stitched_ts_is_the_whole_captures(runs, name):
    ts, _ = runs[name]
    cfg = CONFIGS[name]
    rpk, pk = bc.packets(bc.reference_ts(cfg["args"], 2500, 3, cfg["noise"])), bc.packets(ts)            # (d)
    assert len(rpk) > 2300, f"{name}: invalid input, the reference returns {len(rpk)} packets"
    where = {}
    for j, p in enumerate(rpk):
        where.setdefault(p, j)
    i0 = next(i for i, p in enumerate(pk) if p in where)
    j0 = where[pk[i0]]
    m = min(len(pk) - i0, len(rpk) - j0)
    print(f"{name}: {len(pk)} packets, reference {len(rpk)}, pair at {i0} / {j0}, compared {m}, not reached {len(rpk) - j0 - m}")
    assert pk[i0:i0 + m] == rpk[j0:j0 + m], f"{name}: differs from the whole capture's TS"
    assert len(pk) - i0 == m, f"{name}: {len(pk) - i0 - m} packets behind the reference's last"
    assert len(rpk) - j0 - m <= 8, f"{name}: {len(rpk) - j0 - m} of the reference's last packets not reached"
    assert i0 <= 8 and j0 <= 8, f"{name}: the first common packet is at {i0} / {j0}"


def test_the_references_own_pieces_lose_one_packet(capi):
    """The condition behind (d): the reference binary alone, piece by piece, stitched by the restatement."""
    iq = bc.capture(2500, 3, 7.5)[0]
    plan = capi.recording_plan(len(iq) // 2, PIECE, OVERLAP)
    with ThreadPoolExecutor(max_workers=8) as ex:
        pieces = list(ex.map(lambda p: bc.run_reference(bc.REF_U8, iq[2 * p[0]:2 * (p[0] + p[1])]), plan))
    joins, keep, ts = sc.stitch(pieces, WINDOW, MIN_RUN)
    whole = bc.reference_ts(bc.REF_U8, 2500, 3, 7.5)
    assert all(j["joined"] for j in joins) and min(j["run"] for j in joins) >= 94
    assert ts == whole[:len(whole) - 188] and len(whole) // 188 == 2446


def test_decode_file_is_decode(capi, ctx, runs, tmp_path):
    iq = bc.capture(2500, 3, 7.5)[0]                                                                     # (e)
    path = tmp_path / "capture.cu8"
    iq.tofile(path)
    dec = capi.RecordingDecoder(ctx, PIECE, OVERLAP, 4, omega=1.2, window=WINDOW, min_run=MIN_RUN)
    try:
        ts, report = dec.decode_file(str(path))
        again, _ = dec.decode_file(str(path))                                                            # a reused object, its buffers kept
    finally:
        dec.close()
    want, wanted_report = runs["default, 4 per batch"]
    assert ts == want and again == want
    assert report["joins"] == wanted_report["joins"] and report["tune"] == wanted_report["tune"]


def test_a_piece_of_noise_is_reported_and_costs_nothing_else(capi, ctx):
    iq, sent = bc.capture(2500, 3, 7.5)                                                                  # (f)
    hit = iq.copy()
    hit[2 * 2000000:2 * 3000000] = bc.noise_only(1000000, np.random.default_rng(5))                      # piece 4 of 9, whole
    ts, report = decode(capi, ctx, hit, pieces_per_batch=4)
    produced = [p["result"]["ts_packets"] for p in report["pieces"]]
    print("packets per piece", produced, "joins", [(j["joined"], j["run"]) for j in report["joins"]], "unjoined", report["unjoined"])
    assert produced[4] == 0 and report["unjoined"] == [3, 4]
    # the joins and the kept ranges are the restatement's; where a piece that acquired late holds less in front of the run than its right
    # neighbour, the neighbour's packets go out there
    joins, keep, plain = sc.stitch([p["ts"] for p in report["pieces"]], WINDOW, MIN_RUN)
    heads = [p.get("head_in_front", 0) for p in report["pieces"]]
    print("heads in front", heads, "packets", report["packets"], "plain stitch", len(plain) // 188)
    assert report["joins"] == joins and [p["keep"] for p in report["pieces"]] == [[k["start"], k["end"]] for k in keep]
    dropped = [p.get("dropped_in_front", 0) for p in report["pieces"]]
    assert report["packets"] == len(plain) // 188 + sum(heads) - sum(dropped) and all(d < h for d, h in zip(dropped, heads) if h)
    got = set(bc.packets(ts))
    for k, p in enumerate(report["pieces"]):
        lost = [q for q in bc.packets(p["ts"]) if q in sent and q not in got]
        assert lost == [], f"piece {k}: {len(lost)} of its packets are not in the stitched TS"
    # (a piece that acquires anew in the middle of the stream brings its few packets that are not derandomised yet, as piece 0 does at
    # the start: the counters asked are those of the transmitted packets)
    c = [(q[1] << 16) | (q[2] << 8) | q[3] for q in bc.packets(ts) if q in sent]
    assert len(set(c)) == len(c) and c == sorted(c) and len(c) > 1800
