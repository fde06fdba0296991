"""The C++ host framework (leansdr_amd/host: scheduler / pipebuf / shim blocks with the reference's class surface) driving the
HIP kernels through the C ABI, end to end through the REFERENCE'S OWN graph builder: oracle/_ref/ref_graph/leandvb is
/root/reference/src/apps/leandvb.cc compiled unchanged against this repo's host headers (tests/test_gpu_ref_graph.py checks it
byte for byte against the reference binary; here the transport stream is checked against the oracle chain, for several pipe
sizes and for the throughput modes, which the reference's command line has no option for: they come from the environment,
LSDR_TILED=1).  Symbol-level parity of the same blocks is tests/test_gpu_rx.py / test_gpu_fir.py (goldens of the reference)."""
import os
import sys
import subprocess
import numpy as np
import pytest
from conftest import gold, bits_equal, ROOT
import pyoracle as po

pytestmark = [pytest.mark.gpu]
APP = os.path.join(ROOT, "oracle", "_ref", "ref_graph", "leandvb")


@pytest.fixture(autouse=True, scope="module")
def _receiver_cli_must_exist():
    """The receiver CLI of this repo IS the reference's leandvb.cc compiled against leansdr_amd/host (`make -C oracle ref_graph`,
    done by __graft_entry__.build() where the reference sources are; the binary travels with oracle/_ref).  On a GPU box
    without it every full-chain test of this module would be skipped silently — fail instead."""
    assert os.path.exists(APP), (f"{APP} is missing: build it where the reference sources are (make -C oracle ref_graph, "
                                 "or python -c 'import __graft_entry__ as g; g.build()') — the full-chain tests cannot run without it")
C1 = ["--u8", "-f", "2400e3", "--sr", "2000e3", "--cr", "1/2"]


def run_ts(args, data, tiled=False):
    env = dict(os.environ, LSDR_TILED="1") if tiled else None
    p = subprocess.run([APP] + args, input=data.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180, env=env)
    assert p.returncode == 0, p.stderr.decode()
    return np.frombuffer(p.stdout, np.uint8).reshape(-1, 188), p.stderr.decode()


def after_acquisition(ts, want, skip=16):
    """Every packet of `want` after its first `skip` is in `ts`, byte for byte and in order (lock instants may differ by a few
    packets between the exact and the throughput receivers)."""
    got = [bytes(t) for t in ts]
    tail = [bytes(t) for t in want[skip:]]
    assert tail and tail[0] in got
    i0 = got.index(tail[0])
    return got[i0:i0 + len(tail)] == tail


@pytest.mark.parametrize("buf_factor", [4, 64, 4096])
def test_full_chain_ts_vs_oracle(oracle, buf_factor):
    """u8 capture → TS packets through the whole GPU graph == oracle front end + FEC tail (which tests/test_oracle_fec.py pins
    to the real `leandvb` binary, default algebraic deconvolution), for the reference's pipe sizes and for GPU-sized ones."""
    from leansdr_amd import synth_dvbs
    iq, ts_in = synth_dvbs.capture_u8(n_packets=1000, sps_num=6, sps_den=5, seed=3)
    ts, err = run_ts(C1 + ["--buf-factor", str(buf_factor), "--fd-info", "2"], iq)
    # default --anf 1 like leandvb: a bit-exact pass-through here (no detect within 4 Mi samples) that only
    # withholds the last partial 4096-sample block
    x = oracle.cconverter_u8(iq)
    x = x[: len(x) // 4096 * 4096]
    p = po.rx_params(sampler=1, cstln=1, omega=float(np.float32(2400e3 / 2000e3)), meas_decimation=int(2400e3 / 5))
    want = oracle.fec_chain(oracle.rx(p, x)["sym"], 1, 0, 0)[0]
    assert len(want) > 60
    assert bits_equal(ts, want)
    sent = {bytes(t) for t in ts_in}
    assert sum(bytes(t) in sent for t in ts) >= len(ts) - 10   # a few packets around acquisition are false locks, as in the reference
    assert "LOCK 1" in err


@pytest.mark.parametrize("buf_factor", [4, 256])
def test_full_chain_viterbi_ts_vs_oracle(oracle, buf_factor):
    """--viterbi: cstln_receiver(pll/6) → viterbi_sync → mpeg_sync → deinterleaver → RS → derandomizer on the GPU
    == the oracle chain that tests/test_oracle_fec.py pins to `leandvb --viterbi`."""
    from leansdr_amd import synth_dvbs
    iq, ts_in = synth_dvbs.capture_u8(n_packets=300, sps_num=6, sps_den=5, seed=4)
    ts, _ = run_ts(C1 + ["--viterbi", "--anf", "0", "--buf-factor", str(buf_factor)], iq)
    x = oracle.cconverter_u8(iq)
    p = po.rx_params(sampler=1, cstln=1, omega=float(np.float32(2400e3 / 2000e3)), meas_decimation=int(2400e3 / 5),
                     pll_adjustment=1 / 6.0)
    want = oracle.fec_chain(oracle.rx(p, x)["sym"], 1, 0, 1)[0]
    assert len(want) > 200 and bits_equal(ts, want)
    sent = {bytes(t) for t in ts_in}
    assert sum(bytes(t) in sent for t in ts) >= len(ts) - 2


def test_full_chain_viterbi_noisy_is_exact(oracle):
    """Low SNR: viterbi_sync keeps switching alignments before it locks (exercises the look-ahead budget and the
    verified fix-up rounds); the TS output must still be bit-identical to the oracle chain."""
    from leansdr_amd import synth_dvbs
    iq, _ = synth_dvbs.capture_u8(n_packets=300, sps_num=6, sps_den=5, seed=9, noise_std=25.0)
    ts, _ = run_ts(C1 + ["--viterbi", "--anf", "0"], iq)
    x = oracle.cconverter_u8(iq)
    p = po.rx_params(sampler=1, cstln=1, omega=float(np.float32(2400e3 / 2000e3)), meas_decimation=int(2400e3 / 5),
                     pll_adjustment=1 / 6.0)
    want = oracle.fec_chain(oracle.rx(p, x)["sym"], 1, 0, 1)[0]
    assert bits_equal(ts, want)


@pytest.mark.parametrize("viterbi", [0, 1])
def test_tiled_receiver_ts_matches_exact_chain(oracle, viterbi):
    """LSDR_TILED=1 (the throughput receiver, not bit-exact at the soft-symbol level) must deliver the same transport
    stream as the exact chain once locked."""
    from leansdr_amd import synth_dvbs
    iq, ts_in = synth_dvbs.capture_u8(n_packets=1000, sps_num=6, sps_den=5, seed=5)
    ts, _ = run_ts(C1 + ["--anf", "0", "--buf-factor", "4096"] + (["--viterbi"] if viterbi else []), iq, tiled=True)
    x = oracle.cconverter_u8(iq)
    p = po.rx_params(sampler=1, cstln=1, omega=float(np.float32(2400e3 / 2000e3)), meas_decimation=int(2400e3 / 5),
                     pll_adjustment=1 / 6.0 if viterbi else 1.0)
    want = oracle.fec_chain(oracle.rx(p, x)["sym"], 1, 0, viterbi)[0]
    assert len(want) > 900 and after_acquisition(ts, want)


def test_tiled_rrc_sampler_ts_matches_exact_chain():
    """--sampler rrc in the throughput mode: the transport stream of the exact chain with the same sampler, once locked."""
    from leansdr_amd import synth_dvbs
    iq, _ = synth_dvbs.capture_u8(n_packets=1000, sps_num=6, sps_den=5, seed=5)
    flags = C1 + ["--anf", "0", "--sampler", "rrc", "--buf-factor", "4096"]
    want, _ = run_ts(flags, iq)
    ts, _ = run_ts(flags, iq, tiled=True)
    assert len(want) > 300          # (the matched filter's 1/S gain makes the AGC — hence the lock — slow: SURVEY A5)
    assert after_acquisition(ts, want, skip=len(want) // 2)


@pytest.mark.parametrize("extra", [[], ["--viterbi"]])
def test_full_chain_fastlock(oracle, extra):
    """--fastlock (deconvol_sync scoring all alignments per call, mpeg_sync run_searching_fast, viterbi resync every
    chunk).  Its decisions depend on how the stream is cut into run() calls, so the check is the payload: every packet
    after acquisition is one of the transmitted packets, and at least as many come out as from the oracle chain."""
    from leansdr_amd import synth_dvbs
    iq, ts_in = synth_dvbs.capture_u8(n_packets=600, sps_num=6, sps_den=5, seed=6)
    ts, _ = run_ts(C1 + ["--anf", "0", "--fastlock", "--buf-factor", "4"] + extra, iq)
    x = oracle.cconverter_u8(iq)
    vit = 1 if extra else 0
    p = po.rx_params(sampler=1, cstln=1, omega=float(np.float32(2400e3 / 2000e3)), meas_decimation=int(2400e3 / 5),
                     pll_adjustment=1 / 6.0 if vit else 1.0)
    want = oracle.fec_chain(oracle.rx(p, x)["sym"], 1, 0, vit, fastlock=1)[0]
    sent = {bytes(t) for t in ts_in}
    good = sum(bytes(t) in sent for t in ts)
    assert good >= len(ts) - 10 and len(ts) >= len(want) - 8 and len(ts) > 500


@pytest.mark.parametrize("extra,key", [([], "ts"), (["--fastlock"], "ts_fastlock")])
@pytest.mark.parametrize("buf_factor", [4, 64, 4096])
def test_hs_app_equals_leandvb_hs(extra, key, buf_factor):
    """leandvb --hs on the GPU headers (fast_qpsk_receiver / dvb_deconvol_sync / mpeg_sync(fastlock) / …) == the TS the real
    `leandvb --hs` wrote for the same capture (tests/golden/hs.npz), for any pipe size."""
    g = gold("hs.npz")
    ts, err = run_ts(["--u8", "--hs", "-f", "2400e3", "--sr", "2000e3", "--buf-factor", str(buf_factor), "--fd-info", "2"] + extra, g["iq"])
    assert bits_equal(ts, g[key]) and len(ts) > 20
    assert "LOCK 1" in err   # (no VBER line: the window is max(Fm/2, 50000) bits like the reference's, longer than this capture)


def test_hs_tiled_app_ts_matches_exact_chain(oracle):
    """--hs in the throughput mode: same transport stream as the exact --hs chain once locked."""
    from leansdr_amd import synth_dvbs
    iq, ts_in = synth_dvbs.capture_u8(n_packets=1000, sps_num=6, sps_den=5, seed=5)
    ts, _ = run_ts(["--u8", "--hs", "-f", "2400e3", "--sr", "2000e3", "--buf-factor", "4096"], iq, tiled=True)
    want = oracle.hs_chain(iq, float(np.float32(2400e3 / 2000e3)))
    assert len(want) > 900 and after_acquisition(ts, want)
