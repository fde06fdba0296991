"""Without a GPU: the numpy restatement of lsdr_ts_stitch's definition (stitch_common) on hand-made streams and on the cases the device is
then held to (test_gpu_ts_stitch.py), and the piece plan of capi.RecordingDecoder (capi.recording_plan, capi.overlap_for)."""
import numpy as np
import pytest
import stitch_common as sc


def numbered(lo, hi, pid=0x100):
    """Packets lo … hi − 1 of a stream whose packets carry their number in bytes 4 … 7."""
    p = np.zeros((hi - lo, 188), np.uint8)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = 0x47, pid >> 8, pid & 255, 0x10
    p[:, 4:8] = np.arange(lo, hi, dtype=">u4").view(np.uint8).reshape(-1, 4)
    return p


def test_join_by_hand():
    t, h = numbered(0, 100), numbered(70, 200)
    assert sc.join(t, h, 64, 8) == dict(joined=1, run=30, end=100, next_start=30)
    # the window cuts both sides: T = 80 … 99 and H = 70 … 89 share 80 … 89, and the streams change over behind packet 89
    assert sc.join(t, h, 20, 8) == dict(joined=1, run=10, end=90, next_start=20)
    # windows that do not meet: T = 90 … 99, H = 70 … 79
    assert sc.join(t, h, 10, 8) == dict(joined=0, run=0, end=100, next_start=0)
    assert sc.join(t, numbered(95, 200), 64, 8) == dict(joined=0, run=0, end=100, next_start=0)       # five common packets, M = 8
    assert sc.join(t, numbered(92, 200), 64, 8) == dict(joined=1, run=8, end=100, next_start=8)
    assert sc.join(t[:0], h, 64, 8)["joined"] == 0 and sc.join(t, h[:0], 64, 8) == dict(joined=0, run=0, end=100, next_start=0)
    # a packet lost on the left inside the overlap: runs of 10 (70 … 79) and 19 (81 … 99) on neighbouring diagonals, the longer joins
    lost = np.delete(t, 80, axis=0)
    assert sc.join(lost, h, 64, 8) == dict(joined=1, run=19, end=99, next_start=30)
    # ties go to the smallest a: two runs of 10
    two = np.concatenate([numbered(0, 10), numbered(500, 503), numbered(0, 10)])
    assert sc.join(two, np.concatenate([numbered(0, 10), numbered(900, 950)]), 64, 8) == dict(joined=1, run=10, end=10, next_start=10)


def test_null_packets_do_not_join():
    nulls = sc.null_packets(40)
    t, h = np.concatenate([numbered(0, 50), nulls]), np.concatenate([nulls, numbered(50, 100)])
    assert sc.join(t, h, 64, 8)["joined"] == 0
    # four packets of eight that are not null are enough, three are not
    mixed = lambda k: np.concatenate([numbered(0, k), sc.null_packets(8 - k)])
    assert sc.join(np.concatenate([numbered(100, 130), mixed(4)]), np.concatenate([mixed(4), numbered(200, 230)]), 64, 8)["run"] == 8
    assert sc.join(np.concatenate([numbered(100, 130), mixed(3)]), np.concatenate([mixed(3), numbered(200, 230)]), 64, 8)["joined"] == 0


def test_stitch_by_hand():
    streams = [numbered(0, 100), numbered(70, 180), numbered(150, 160), numbered(158, 300)]
    joins, keep, ts = sc.stitch(streams, 64, 8)
    assert [j["joined"] for j in joins] == [1, 1, 0]                      # the last overlap has two packets
    assert keep == [dict(start=0, end=100, out_offset=0), dict(start=30, end=90, out_offset=100), dict(start=10, end=10, out_offset=160),
                    dict(start=0, end=142, out_offset=160)]
    assert ts == np.concatenate([numbered(0, 160), numbered(158, 300)]).tobytes()       # nothing dropped where nothing joined
    # a stream shorter than both of its overlaps keeps nothing: 40 … 59 lies inside 0 … 99 and 30 … 199
    joins, keep, ts = sc.stitch([numbered(0, 60), numbered(40, 60), numbered(30, 40), numbered(300, 400)], 64, 8)
    assert keep[1]["start"] == keep[1]["end"] == 20
    assert sc.stitch([numbered(0, 10)], 64, 8) == ([], [dict(start=0, end=10, out_offset=0)], numbered(0, 10).tobytes())
    assert sc.stitch([numbered(0, 0), numbered(0, 0)], 64, 8)[2] == b""


@pytest.mark.parametrize("k", range(len(sc.cases())), ids=[c[0] for c in sc.cases()])
def test_cases_are_what_they_say(k):
    name, streams, joined = sc.cases()[k]
    assert len(streams) == 4 and all(len(s) <= sc.MAX_PACKETS for s in streams), name
    joins, keep, ts = sc.stitch(streams)
    print(name, joins, keep)
    assert [j["joined"] for j in joins] == joined, (name, joins)
    assert len(ts) == 188 * sum(r["end"] - r["start"] for r in keep)
    if name in ("plain overlaps", "deleted on the right", "a stream shorter than W"):
        # the stitched stream is the stream the pieces were cut from (its packets 0 … the last piece's end), every packet once
        b = sc.base()
        assert ts == b[:len(ts) // 188].tobytes() and len(ts) // 188 >= 2400, name
    if name == "a stream its joins consume":
        assert keep[1]["start"] == keep[1]["end"], keep
    if name == "a periodic stretch":
        assert joins[0]["run"] == 100, joins                               # not the twelve packets on the other diagonal
    if name == "one bit changed inside the overlap":
        assert joins[0]["run"] == 50, joins


def test_plan(capi):
    plan = capi.recording_plan
    for n, piece, overlap in ((4896023, 1000000, 500000), (4896023, 1000000, 300000), (4896023, 1000000, 800000), (10 * 8192, 8192, 4096),
                              (8192 * 3 + 1, 8192, 4096), (100, 8192, 4096), (0, 8192, 4096), (8192, 8192, 0), (8193, 8192, 0), (4097, 8192, 4096)):
        p = plan(n, piece, overlap)
        stride = piece - overlap
        assert len(p) == max(1, -(-(n - overlap) // stride)), (n, piece, overlap)
        assert [s for s, _ in p] == [i * stride for i in range(len(p))] and all(s % 8 == 0 for s, _ in p)
        assert all(length == piece for _, length in p[:-1]) and 0 <= p[-1][1] <= piece
        assert p[-1][0] + p[-1][1] == n and (n == 0 or p[-1][1] > 0)                                   # the pieces cover [0, n)
        for (s0, l0), (s1, _) in zip(p, p[1:]):
            assert s0 + l0 - s1 == overlap                                                            # adjacent pieces share exactly `overlap`
    assert len(plan(4896023, 1000000, 500000)) == 9 and len(plan(4896023, 1000000, 300000)) == 7 and len(plan(4896023, 1000000, 800000)) == 21
    assert plan(100, 8192, 4096) == [(0, 100)] and plan(0, 8192, 4096) == [(0, 0)] and plan(16384, 8192, 4096) == [(0, 8192), (4096, 8192), (8192, 8192)]
    for bad in ((8192, 8192), (8192, 9000), (8190, 4096), (8192, 4095), (8192, -8)):
        with pytest.raises(capi.LsdrError):
            plan(1000, *bad)


def test_overlap_for(capi):
    # 255 packets of 1632 symbols at 1.2 samples per symbol: 499 392 samples, rounded up to 122 · 4096
    assert capi.overlap_for(capi.FEC12, 1.2, packets=255) == 499712
    assert capi.overlap_for(capi.FEC78, 1.2, packets=100) == -(-int(np.ceil(100 * 204 * 8 * 8 / 14 * 1.2)) // 4096) * 4096
    for fec, lost in capi.ACQUISITION_PACKETS.items():
        num, den = capi.FEC_RATE[fec]
        got = capi.overlap_for(fec, 1.2, window=256)
        assert got % 4096 == 0 and 0 <= got - (lost + 256) * 1632 * den / (2 * num) * 1.2 < 4096
    assert capi.overlap_for(capi.FEC12, 1.2) == capi.overlap_for(capi.FEC12, 1.2, packets=capi.ACQUISITION_PACKETS[capi.FEC12] + 4096)
    with pytest.raises(capi.LsdrError):
        capi.overlap_for(capi.FEC910, 1.2)
