"""lsdr_viterbi_batch: B independent viterbi_sync decoders in shared launches, decisions and repair on the device.
The expected value is always the CPU oracle's viterbi_sync of each stream ALONE (bytes, total consumed, final alignment);
the only tolerance is equality."""
import ctypes as C
import hashlib
import numpy as np
import pytest
from conftest import bits_equal
from fec_common import fec_input, hard_symbols

pytestmark = pytest.mark.gpu

KERNEL_HOOKS = ("LSDR_VIT_Q4", "LSDR_VIT_LANE", "LSDR_VIT_GENERIC")
ALL_HOOKS = KERNEL_HOOKS + ("LSDR_VIT_WO", "LSDR_VITB_ROUNDS", "LSDR_VIT_TL", "LSDR_VIT_HOST_REPAIR")


@pytest.fixture(params=["auto", "q4", "lane", "generic"])
def vit_kernel(request, monkeypatch):
    """The four kernel selections of the single-stream tests: the batch honours the same hooks."""
    for k in ALL_HOOKS:
        monkeypatch.delenv(k, raising=False)
    if request.param != "auto":
        monkeypatch.setenv({"q4": "LSDR_VIT_Q4", "lane": "LSDR_VIT_LANE", "generic": "LSDR_VIT_GENERIC"}[request.param], "1")
    return request.param


@pytest.fixture
def no_hooks(monkeypatch):
    for k in ALL_HOOKS:
        monkeypatch.delenv(k, raising=False)


_want = {}


def want_of(oracle, sym, cstln=1, rate=0, period=0):
    """oracle.viterbi_sync of one stream alone (cached: several cases share streams)."""
    key = (hashlib.sha256(np.ascontiguousarray(sym).tobytes()).hexdigest(), cstln, rate, period)
    if key not in _want:
        _want[key] = oracle.viterbi_sync(sym, cstln, rate, period)
    return _want[key]


def mixed_streams():
    """Case 1's batch: four noise levels, the three relabelled streams of test_viterbi_alignment_search (streams 2, 4, 6), one stream
    shorter than a chunk."""
    hard = hard_symbols()
    rot = np.array([2, 0, 3, 1], np.uint8)       # +90° relabelling
    conj = np.array([1, 0, 3, 2], np.uint8)
    e = {x: fec_input(hard, x) for x in (0, 40, 120, 300)}
    return [e[0], e[40], fec_input(rot[hard], 40), e[120], fec_input(conj[hard], 40), e[300], fec_input(rot[conj][hard], 40), e[0][:100]]


RELABELLED = (2, 4, 6)


def check_streams(oracle, got, syms, cstln=1, rate=0, period=0):
    for i, ((vb, cons, cur), sym) in enumerate(zip(got, syms)):
        want, wcons, wcur = want_of(oracle, sym, cstln, rate, period)
        print(f"stream {i}: {len(sym)} symbols -> consumed {cons} (oracle {wcons}), {len(vb)} bytes (oracle {len(want)}), alignment {cur} (oracle {wcur})")
        assert cons == wcons and cur == wcur, (i, cons, wcons, cur, wcur)
        assert bits_equal(vb, want), i


def drive(ctx, vb, syms, only_runs=None):
    """run_async -> wait until no stream makes progress (or for `only_runs` runs), every stream advanced by its own `consumed`; keeps
    every run's records.  Returns (bytes per stream, records per run)."""
    syms = [np.ascontiguousarray(s, vb_softsym()) for s in syms]
    cap = max(len(s) for s in syms) + 64
    dins = [ctx.upload(s) for s in syms]
    douts = [ctx.alloc(cap) for _ in syms]
    pos, nout, log = [0] * len(syms), [0] * len(syms), []
    for _ in range(only_runs or 100000):
        vb.run_async_dev([d.at(p * 4) for d, p in zip(dins, pos)], [len(s) - p for s, p in zip(syms, pos)],
                         [d.at(o) for d, o in zip(douts, nout)], cap - max(nout))
        res = vb.wait()
        log.append(res)
        for i, r in enumerate(res):
            pos[i] += r["consumed"]
            nout[i] += r["produced"]
        if not any(r["consumed"] for r in res):
            break
    else:
        assert only_runs, "the batch did not terminate"
    out = [ctx.download(d, np.uint8, n) if n else np.empty(0, np.uint8) for d, n in zip(douts, nout)]
    for d in dins + douts:
        d.free()
    return out, log


def vb_softsym():
    from fec_common import SOFTSYM
    return SOFTSYM


# ---------------------------------------------------------------- 1. mixed batch
def test_mixed_batch_qpsk12(capi, ctx, oracle, vit_kernel):
    syms = mixed_streams()
    vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, len(syms), max(len(s) for s in syms))
    got, runs = vb.run_streams(syms)
    vb.close()
    print("kernel", vit_kernel, "runs", runs)
    check_streams(oracle, got, syms)
    for i in RELABELLED:
        assert got[i][2] != 0
    assert got[7][1] == 0 and len(got[7][0]) == 0


# ---------------------------------------------------------------- 2. other codes
def test_8psk23_three_seeds_one_batch(capi, ctx, oracle, vit_kernel):
    syms = []
    for seed, maxcost in [(5, 9000), (6, 3), (7, 32768)]:      # the streams of test_viterbi_8psk23_kernels_vs_oracle
        rng = np.random.default_rng(seed)
        n = 120000
        sym = np.zeros(n, capi.SOFTSYM)
        sym["symbol"] = rng.integers(0, 8, n)
        sym["cost"] = np.maximum(-rng.integers(0, maxcost + 1, n), -32768)
        syms.append(sym)
    vb = capi.ViterbiBatch(ctx, capi.PSK8, capi.FEC23, 3, 120000)
    got, runs = vb.run_streams(syms)
    vb.close()
    check_streams(oracle, got, syms, 2, 1)


@pytest.mark.parametrize("rate,period", [(3, 0), (2, 0), (3, 1), (4, 0), (5, 0)])
def test_generic_kernel_nshifts(capi, ctx, oracle, no_hooks, rate, period):
    """QPSK 3/4 (two symbols per FEC block), 4/6 (three), 5/6 (three) and 7/8 (four): the table-driven kernel, alignments that differ by a
    symbol shift."""
    syms = []
    for seed in (4, 11):
        rng = np.random.default_rng(seed)
        sym = np.zeros(50000, capi.SOFTSYM)
        sym["symbol"] = rng.integers(0, 4, 50000)
        sym["cost"] = -rng.integers(0, 9000, 50000)
        syms.append(sym)
    vb = capi.ViterbiBatch(ctx, capi.QPSK, rate, 2, 50000, resync_period=period)
    got, runs = vb.run_streams(syms)
    vb.close()
    check_streams(oracle, got, syms, 1, rate, period)


# ---------------------------------------------------------------- 3. independence
def test_stream_is_independent_of_its_neighbours(capi, ctx, oracle, no_hooks):
    sym = mixed_streams()[0]
    one = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, 1, len(sym))
    a, loga = drive(ctx, one, [sym])
    one.close()
    rng = np.random.default_rng(21)
    others = []
    for k in range(7):
        s = np.zeros(len(sym) - 1000 * k, capi.SOFTSYM)
        s["symbol"] = rng.integers(0, 4, len(s))
        s["cost"] = -rng.integers(0, 9000, len(s))
        others.append(s)
    syms = others[:5] + [sym] + others[5:]
    many = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, 8, len(sym))
    b, logb = drive(ctx, many, syms)
    many.close()
    ca = [r[0]["consumed"] for r in loga]
    cb = [r[5]["consumed"] for r in logb]
    while ca and ca[-1] == 0:
        ca.pop()
    while cb and cb[-1] == 0:
        cb.pop()
    print("consumed per call, alone:", ca, "in the batch:", cb)
    assert ca == cb
    assert bits_equal(a[0], b[5])
    assert bits_equal(a[0], want_of(oracle, sym)[0])


# ---------------------------------------------------------------- 4. cutting
@pytest.mark.parametrize("pipe", [4096, 40000])
def test_windows_give_the_same_bytes(capi, ctx, oracle, no_hooks, pipe):
    syms = mixed_streams()
    vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, len(syms), max(len(s) for s in syms))
    got, runs = vb.run_streams(syms, pipe=pipe)
    vb.close()
    print("pipe", pipe, "runs", runs)
    check_streams(oracle, got, syms)


# ---------------------------------------------------------------- 5. device-side counts
def test_device_side_counts(capi, ctx, oracle, no_hooks):
    syms = mixed_streams()
    lens = [len(s) for s in syms]
    limit = [lens[0] // 2, lens[1], 0, lens[3] // 2, lens[4], lens[5], lens[6] // 2, lens[7]]
    vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, len(syms), max(lens))
    got, runs = vb.run_streams(syms, n_in_dev=limit)
    vb.close()
    check_streams(oracle, got, [s[:m] for s, m in zip(syms, limit)])
    assert got[2][1] == 0 and len(got[2][0]) == 0


# ---------------------------------------------------------------- 6. repair and stall
@pytest.mark.parametrize("kernel,copies", [("auto", 41), ("lane", 6)])
def test_repair_on_the_device_and_stall_without_it(capi, ctx, oracle, monkeypatch, kernel, copies):
    """LSDR_VIT_WO=1: the other alignments' tiles warm up over ONE resync chunk, so many of their seams fail (the input of
    test_viterbi_repair_round).  With the repair rounds the device decodes those tiles again; with the rounds forced to zero the
    streams stall in front of the first such seam and need more runs — exact bytes either way, because only verified work is committed."""
    for k in ALL_HOOKS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LSDR_VIT_WO", "1")
    if kernel == "lane":
        monkeypatch.setenv("LSDR_VIT_LANE", "1")
    sym = fec_input(np.tile(hard_symbols(), copies), 120)
    want, wcons, wcur = want_of(oracle, sym)
    syms = [sym] * 4
    vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, 4, len(sym))
    got, log = drive(ctx, vb, syms)
    repaired = sum(r["repaired"] for res in log for r in res)
    stalled = sum(r["stalled"] for res in log for r in res)
    print(kernel, "with repair rounds: runs", len(log), "repaired", repaired, "stalled", stalled)
    for i in range(4):
        assert sum(res[i]["consumed"] for res in log) == wcons and log[-1][i]["current_sync"] == wcur
        assert bits_equal(got[i], want), i
    assert repaired > 0
    vb.reset(-1)
    monkeypatch.setenv("LSDR_VITB_ROUNDS", "0")
    got0, log0 = drive(ctx, vb, syms)
    vb.close()
    repaired0 = sum(r["repaired"] for res in log0 for r in res)
    stalled0 = sum(r["stalled"] for res in log0 for r in res)
    print(kernel, "without repair rounds: runs", len(log0), "repaired", repaired0, "stalled", stalled0)
    for i in range(4):
        assert sum(res[i]["consumed"] for res in log0) == wcons and log0[-1][i]["current_sync"] == wcur
        assert bits_equal(got0[i], want), i
    assert repaired0 == 0 and stalled0 > 0 and len(log0) > len(log)


# ---------------------------------------------------------------- 7. reset and reuse
def test_reset_and_reuse(capi, ctx, oracle, no_hooks):
    syms = mixed_streams()
    vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, len(syms), max(len(s) for s in syms))
    first, _ = vb.run_streams(syms)
    vb.reset(-1)
    again, _ = vb.run_streams(syms)
    check_streams(oracle, again, syms)
    for a, b in zip(first, again):
        assert bits_equal(a[0], b[0]) and a[1:] == b[1:]
    # reset(2) between two halves: stream 2 (relabelled) starts over from alignment 0 with fresh decoders, the others carry on
    vb.reset(-1)
    cut = 700 * 128
    heads = [s[:cut] for s in syms]
    tails = [s[cut:] for s in syms]
    h, _ = vb.run_streams(heads)
    assert [x[1] for x in h[:7]] == [cut] * 7
    vb.reset(2)
    t, _ = vb.run_streams(tails)
    vb.close()
    for i in range(7):
        if i == 2:
            want, wcons, wcur = want_of(oracle, tails[2])
            assert wcur != 0
            assert t[2][1] == wcons and t[2][2] == wcur and bits_equal(t[2][0], want)
        else:
            want, wcons, wcur = want_of(oracle, syms[i])
            assert cut + t[i][1] == wcons and t[i][2] == wcur, i
            assert bits_equal(np.concatenate([h[i][0], t[i][0]]), want), i


# ---------------------------------------------------------------- 8. shared launches
def test_launches_do_not_depend_on_the_number_of_streams(capi, ctx, oracle, no_hooks):
    sym = mixed_streams()[1]
    launches = {}
    for B in (1, 32):
        vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, B, len(sym))
        got, runs = vb.run_streams([sym] * B)
        check_streams(oracle, got, [sym] * B)
        vb.reset(-1)
        _, log = drive(ctx, vb, [sym] * B, only_runs=1)      # a run with work for every stream
        st = vb.stats()
        vb.close()
        assert all(r["consumed"] > 0 for r in log[0])
        launches[B] = st["launches_last_run"]
        print("B", B, "runs", runs, st)
    assert launches[1] == launches[32] and launches[1] > 0


def test_locked_stream_is_committed_by_one_run(capi, ctx, oracle, no_hooks):
    sym = fec_input(np.tile(hard_symbols(), 41), 40)
    want, wcons, wcur = want_of(oracle, sym)
    vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, 1, len(sym))
    got, log = drive(ctx, vb, [sym])
    vb.close()
    print("runs", len(log), log[0][0])
    assert log[0][0]["consumed"] == wcons and not log[0][0]["switched"] and not log[0][0]["stalled"]
    assert log[0][0]["current_sync"] == wcur and bits_equal(got[0], want)


# ---------------------------------------------------------------- 9. arguments
def test_arguments(capi, ctx, no_hooks):
    lib = capi.lib
    h = C.c_void_p()
    assert lib.lsdr_viterbi_batch_create(ctx.h, capi.QPSK, capi.FEC12, 0, 1000, C.byref(h)) == -2          # LSDR_E_ARG
    # unsupported (constellation, rate): what lsdr_viterbi_create returns for the same pair
    for cstln, rate in [(capi.QPSK, capi.FEC89), (capi.PSK8, capi.FEC12)]:
        hv = C.c_void_p()
        want = lib.lsdr_viterbi_create(ctx.h, cstln, rate, C.byref(hv))
        assert want < 0
        assert lib.lsdr_viterbi_batch_create(ctx.h, cstln, rate, 2, 1000, C.byref(h)) == want, (cstln, rate)
    sym = mixed_streams()[0][:4096]
    vb = capi.ViterbiBatch(ctx, capi.QPSK, capi.FEC12, 2, 4096)
    din, dout = ctx.upload(sym), ctx.alloc(2 * 4096 + 64)
    ins, ok_outs = [din.at(0), din.at(0)], [dout.at(0), dout.at(4096)]
    with pytest.raises(capi.LsdrError):                                 # misaligned out
        vb.run_async_dev(ins, [4096, 4096], [dout.at(0), dout.at(4097)], 4096)
    with pytest.raises(capi.LsdrError):                                 # more symbols than the object was created for
        vb.run_async_dev(ins, [4096, 4097], ok_outs, 4096)
    with pytest.raises(capi.LsdrError):                                 # nothing in flight
        vb.wait()
    vb.run_async_dev(ins, [4096, 4096], ok_outs, 4096)
    with pytest.raises(capi.LsdrError):                                 # one run in flight per object
        vb.run_async_dev(ins, [4096, 4096], ok_outs, 4096)
    res = vb.wait()
    assert [r["consumed"] for r in res] == [4096, 4096]
    vb.close()
    din.free(); dout.free()
