"""lsdr_hs_each_run_async: every capture of an `--hs` batch with its own length and its own tune, with and without fastlock.

  * ragged lengths: one batch of four lengths of the same capture, every TS against the reference BINARY's (`leandvb … --hs [--fastlock]`);
  * composition invariance, bit for bit: five lengths (long, short, one chunk, one sample short of a chunk, none) tuned differently in one
    batch against the same five as the only capture of a one-capture object through lsdr_hs_batch_run_async with cfg.freq = tune — TS,
    result record and hard symbols — and again in reverse order on the same object;
  * tuning: four carrier offsets, three of them outside the tiles' window, each tuned to its offset, against `leandvb --hs --tune`.

The reference binary (oracle/_ref/leandvb) is required: where it is missing these tests FAIL.
"""
import pytest
from batch_common import REF_U8, capture, check_against_reference, references, shifted

pytestmark = pytest.mark.gpu

OMEGA = 1.2
FS = 2400e3
NOISE = 7.5
N_ALL = 1958423
LENGTHS = [1958423, 1500001, 1000000, 700001]
REF_PACKETS = {0: [956, 722, 467, 314], 1: [986, 752, 497, 344]}      # what the reference returns for LENGTHS, by fastlock
FREQS = [0.0, 1e-3, -1e-3, 3e-3]
REF_PACKETS_TUNED = {0: 956, 1: 986}
LENGTHS5 = [1958423, 700001, 129, 128, 0]
TUNES5 = [1e-3, 0.0, -1e-3, 1e-3, 3e-3]


def _iq():
    iq, sent = capture(1000, 11, NOISE)
    assert len(iq) == 2 * N_ALL
    return iq, sent


def _args(fastlock):
    return REF_U8 + (("--hs", "--fastlock") if fastlock else ("--hs",))


@pytest.mark.parametrize("fastlock", [0, 1])
def test_ragged_lengths_against_the_reference(capi, ctx, fastlock):
    iq, sent = _iq()
    refs = references([(_args(fastlock), 1000, 11, NOISE, n) for n in LENGTHS])
    buf = ctx.upload(iq)
    hb = capi.HsBatch(ctx, len(LENGTHS), N_ALL, OMEGA, fastlock=fastlock)
    try:
        res, ts = hb.decode_each([buf.ptr] * len(LENGTHS), LENGTHS)
    finally:
        hb.close()
        buf.free()
    for i, n in enumerate(LENGTHS):
        check_against_reference(ts[i], refs[i], sent, REF_PACKETS[fastlock][i] - 10, f"fastlock {fastlock} length {n}", True)
        r = res[i]
        assert r["samples"] == (n - 1) // 128 * 128 and r["locked"] == 1 and r["seam_bad"] == 0, (n, r)
    assert len({r["tiles"] for r in res}) == len(LENGTHS)


@pytest.mark.parametrize("fastlock", [0, 1])
def test_composition_invariance(capi, ctx, fastlock):
    iq = _iq()[0]
    bufs = {f: ctx.upload(shifted(iq, f)) for f in sorted(set(TUNES5))}
    B = len(LENGTHS5)
    try:
        alone = []
        for n, f in zip(LENGTHS5, TUNES5):
            hb = capi.HsBatch(ctx, 1, N_ALL, OMEGA, freq=f, fastlock=fastlock)
            try:
                res, ts = hb.decode([bufs[f].ptr], n)
                alone.append((res[0], ts[0], hb.symbols(0, res[0]["symbols"]).tobytes()))
            finally:
                hb.close()
        # conditions on the input: the long captures decode (tuned), one chunk gives symbols, less than a chunk gives nothing
        assert alone[0][0]["ts_packets"] > 900 and alone[1][0]["ts_packets"] > 250, (alone[0][0], alone[1][0])
        assert alone[2][0]["samples"] == 128 and alone[2][0]["symbols"] > 90 and alone[3][0]["symbols"] == 0 and alone[4][0]["symbols"] == 0
        hb = capi.HsBatch(ctx, B, N_ALL, OMEGA, freq=0.25, fastlock=fastlock)      # (cfg.freq is replaced by every capture's tune)
        try:
            for order in (list(range(B)), list(reversed(range(B)))):
                ptrs = [bufs[TUNES5[k]].ptr if LENGTHS5[k] else None for k in order]
                res, ts = hb.decode_each(ptrs, [LENGTHS5[k] for k in order], [TUNES5[k] for k in order])
                for i, k in enumerate(order):
                    name = f"fastlock {fastlock} length {LENGTHS5[k]} tune {TUNES5[k]} at place {i}"
                    assert res[i] == alone[k][0], (name, res[i], alone[k][0])
                    assert ts[i] == alone[k][1], f"{name}: TS"
                    assert hb.symbols(i, res[i]["symbols"]).tobytes() == alone[k][2], f"{name}: symbols"
        finally:
            hb.close()
    finally:
        for b in bufs.values():
            b.free()


@pytest.mark.parametrize("fastlock", [0, 1])
def test_tuning_against_the_reference(capi, ctx, fastlock):
    iq, sent = _iq()
    refs = references([(_args(fastlock) + ("--tune", repr(f * FS)), 1000, 11, NOISE, None, f) for f in FREQS])
    bufs = [ctx.upload(shifted(iq, f)) for f in FREQS]
    hb = capi.HsBatch(ctx, len(FREQS), N_ALL, OMEGA, fastlock=fastlock)
    try:
        res, ts = hb.decode_each([b.ptr for b in bufs], [N_ALL] * len(FREQS), FREQS)
    finally:
        hb.close()
        for b in bufs:
            b.free()
    for i, f in enumerate(FREQS):
        check_against_reference(ts[i], refs[i], sent, REF_PACKETS_TUNED[fastlock] - 10, f"fastlock {fastlock} offset {f} tuned", True)
        assert res[i]["locked"] == 1 and res[i]["seam_bad"] == 0, res[i]


def test_arguments(capi, ctx):
    buf = ctx.upload(_iq()[0][: 2 << 16])
    hb = capi.HsBatch(ctx, 2, 1 << 16, OMEGA)
    run, ptrs = capi.lib.lsdr_hs_each_run_async, hb._ptrs([buf.ptr, buf.ptr])
    try:
        for what, change in (("samples", lambda e: setattr(e[1], "n_samples", (1 << 16) + 1)), ("tune", lambda e: setattr(e[0], "tune", float("nan"))),
                             ("tune", lambda e: setattr(e[0], "tune", -0.5)), ("reserved", lambda e: e[1].reserved.__setitem__(0, 7))):
            e = hb.each([1 << 16, 1000])
            change(e)
            assert run(hb.h, ptrs, e) == -2 and what in capi.lib.lsdr_last_error().decode(), what
        hb.run_each_async([buf.ptr, None], [1 << 16, 0])
        assert run(hb.h, ptrs, hb.each([1 << 16, 1000])) == -2 and "in flight" in capi.lib.lsdr_last_error().decode()
        first = hb.wait()
        res, _ = hb.decode_each([buf.ptr, None], [1 << 16, 0])
        assert res == first and res[0]["symbols"] > 50000 and res[1]["symbols"] == 0 and res[1]["samples"] == 0
    finally:
        hb.close()
        buf.free()
