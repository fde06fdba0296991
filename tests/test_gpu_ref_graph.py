"""The drop-in boundary, tried for real (north_star: "the existing leandvb graph drops in unchanged").

oracle/_ref/ref_graph/{leandvb,leandvbtx,leanchansim,leantsgen} are the REFERENCE'S OWN app sources
(the reference's src/apps/*.cc, compiled where they lie, unmodified, by oracle/Makefile) built against this repo's
host headers instead of the reference's: the same graph-building code, the same three-argument pipebufs, host file_reader /
file_writer / printers — and every DSP/FEC block a GPU block behind the C ABI.  Pipes with a host end and a device end carry
their items over PCIe by themselves (framework.h).  The binaries live under oracle/_ref and travel with it (built artefacts,
git-ignored); where they are missing the tests are skipped, not faked."""
import hashlib
import os
import subprocess
import sys
import numpy as np
import pytest
from conftest import gold, bits_equal, ROOT

pytestmark = pytest.mark.gpu
RG = os.path.join(ROOT, "oracle", "_ref", "ref_graph")
need_graph = pytest.mark.skipif(not os.path.exists(os.path.join(RG, "leandvb")), reason="ref_graph binaries not built (no /root/reference on the build machine)")

BENCH_CASES = [("sps12", "6/5", 18, "", 700), ("sps4_viterbi_rrc", "4", 5.5, "--viterbi --sampler rrc", 500),
               ("sps12_hs", "6/5", 15, "--u8 --hs", 700)]


@need_graph
@pytest.mark.parametrize("name,ratio,snr,flags,npk", BENCH_CASES)
def test_reference_apps_on_gpu_blocks_reproduce_the_reference(name, ratio, snr, flags, npk):
    """test/leandvb_bench.sh's pipeline — leandvbtx | leanchansim --deterministic > file; leandvb --fd-info 2 < file — run
    with the three reference programs compiled against the GPU headers: report text and transport stream are those of the
    reference binaries (tests/golden/bench_sh.npz), digit for digit."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import leandvb_bench as lb
    lb.RX_EXTRA = ""
    g = gold("bench_sh.npz")
    text, ts = lb.run_pipeline(ratio, snr, flags, npk, ref="graph")
    assert len(ts) // 188 == int(g[name + "_ts_n"]) and hashlib.sha256(ts).digest() == bytes(g[name + "_ts_sha"])
    assert text == bytes(g[name + "_info"]).decode()


@need_graph
def test_reference_leandvb_big_pipes_and_throughput_mode(oracle):
    """The same unmodified program with the reference's own --buf-factor option raised (pipes of 16 Mi samples instead of
    16 Ki: what a GPU wants) and, through the environment, the throughput receiver: the transport stream is the exact
    chain's in both cases."""
    import pyoracle as po
    from leansdr_amd import synth_dvbs
    iq, ts_in = synth_dvbs.capture_u8(n_packets=1000, sps_num=6, sps_den=5, seed=5)
    x = oracle.cconverter_u8(iq)
    p = po.rx_params(sampler=1, cstln=1, omega=float(np.float32(2400e3 / 2000e3)), meas_decimation=int(2400e3 / 5))
    want = oracle.fec_chain(oracle.rx(p, x)["sym"], 1, 0, 0)[0]
    cmd = [os.path.join(RG, "leandvb"), "--u8", "-f", "2400e3", "--sr", "2000e3", "--cr", "1/2", "--anf", "0", "--buf-factor", "4096"]
    r = subprocess.run(cmd, input=iq.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    assert r.returncode == 0, r.stderr.decode()
    ts = np.frombuffer(r.stdout, np.uint8).reshape(-1, 188)
    assert len(want) > 900 and bits_equal(ts, want)
    r = subprocess.run(cmd, input=iq.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180, env=dict(os.environ, LSDR_TILED="1"))
    assert r.returncode == 0, r.stderr.decode()
    got = [bytes(t) for t in np.frombuffer(r.stdout, np.uint8).reshape(-1, 188)]
    tail = [bytes(t) for t in want[16:]]
    assert tail[0] in got
    i0 = got.index(tail[0])
    assert got[i0:i0 + len(tail)] == tail


@need_graph
@pytest.mark.parametrize("fmt,dtype,zero", [("--s8", np.int8, 0), ("--u16", np.uint16, 32768), ("--s16", np.int16, 0)])
def test_reference_leandvb_other_input_formats(oracle, fmt, dtype, zero):
    """--s8 / --u16 / --s16 (cconverter<s8|u16|s16,…>, leandvb.cc:218-248): the same capture re-expressed in each integer
    format decodes to the transport stream of the u8 run."""
    from leansdr_amd import synth_dvbs
    iq, _ = synth_dvbs.capture_u8(n_packets=300, sps_num=6, sps_den=5, seed=8)
    base = [os.path.join(RG, "leandvb"), "-f", "2400e3", "--sr", "2000e3", "--cr", "1/2", "--anf", "0"]
    r0 = subprocess.run(base + ["--u8"], input=iq.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    assert r0.returncode == 0 and len(r0.stdout) > 200 * 188, r0.stderr.decode()
    x = (iq.astype(np.int32) - 128 + zero).astype(dtype)          # same sample values around the format's zero
    r1 = subprocess.run(base + [fmt], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    assert r1.returncode == 0, r1.stderr.decode()
    assert r1.stdout == r0.stdout


# ---- same command line, same bytes: the reference's leandvb binary vs its source on the GPU headers ----------------------
REFBIN = os.path.join(ROOT, "oracle", "_ref", "leandvb")
need_both = pytest.mark.skipif(not (os.path.exists(os.path.join(RG, "leandvb")) and os.path.exists(REFBIN)),
                               reason="needs oracle/_ref/ref_graph/leandvb and oracle/_ref/leandvb (built where the reference sources are)")
C1 = ["--u8", "-f", "2400e3", "--sr", "2000e3", "--cr", "1/2"]


def _run_both(flags, data, tmp_path, extra_fd=False, gpu_env=None):
    outs = []
    for exe in (REFBIN, os.path.join(RG, "leandvb")):
        pp = tmp_path / ("pp_" + os.path.basename(os.path.dirname(exe)))
        cmd = " ".join([exe] + flags) + (f" 3>{pp}" if extra_fd else "")
        env = dict(os.environ, **gpu_env) if gpu_env and exe != REFBIN else None
        r = subprocess.run(cmd, shell=True, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        assert r.returncode == 0, (cmd, r.stderr.decode()[-1500:])
        outs.append((r.stdout, pp.read_bytes() if extra_fd else b"", r.stderr.decode()))
    return outs


@need_both
@pytest.mark.parametrize("extra", [[], ["--viterbi"], ["--viterbi", "--hard-metric"], ["--sampler", "nearest"], ["--sampler", "rrc"],
                                   ["--fastlock"], ["--derotate", "3000"], ["--decim", "1", "--anf", "2"], ["--tune", "2000"],
                                   ["--hs"], ["--anf", "0", "--fd-info", "2", "--fd-const", "2", "--fd-spectrum", "2"]],
                         ids=lambda e: "_".join(x.strip("-") for x in e) or "default")
def test_same_command_line_same_bytes_u8(extra, tmp_path):
    """Every hot-path variant of the leandvb command line (leandvb.cc:1100-1250) on a C1-shaped capture: the reference binary
    and the reference SOURCE compiled against the GPU headers write the same transport stream (and the same report text)."""
    from leansdr_amd import synth_dvbs
    iq, _ = synth_dvbs.capture_u8(n_packets=500, sps_num=6, sps_den=5, seed=12)
    (ts_ref, _, err_ref), (ts_gpu, _, err_gpu) = _run_both(C1 + extra, iq.tobytes(), tmp_path)
    if "nearest" not in extra:          # (nearest-sample "interpolation" cannot lock at 1.2 samples/symbol: the reference writes nothing either)
        assert len(ts_ref) > 150 * 188
    assert ts_gpu == ts_ref
    if "--fd-info" in extra:
        assert err_gpu == err_ref


@need_both
def test_same_command_line_same_bytes_f32_resample_fd_pp(tmp_path):
    """Config-2-shaped input (cf32, 120 samples/symbol) with the reference's DEFAULT front end — `--anf 1` and `--resample`
    (auto_notch → fir_filter(313, /30)) — and `--fd-pp 3` (leandvb.cc:418-423): the preprocessed stream the receiver sees is
    byte-identical to the reference's, and so is the transport stream (the a4+a6 end-to-end pin)."""
    from leansdr_amd import synth
    x, _ = synth.qpsk_baseband(120 * 40000, 120, seed=4, rms=1.0, snr_db=15.0, circular=False)
    t = np.arange(len(x))
    x = (x + 2.0 * np.exp(2j * np.pi * 0.0031 * t)).astype(np.complex64)         # a CW interferer inside the filter's passband edge
    flags = ["--f32", "--float-scale", "75", "-f", "240e6", "--sr", "2000e3", "--cr", "1/2", "--resample", "--fd-pp", "3"]
    (ts_ref, pp_ref, _), (ts_gpu, pp_gpu, _) = _run_both(flags, x.tobytes(), tmp_path, extra_fd=True)
    assert len(pp_ref) > 100000 * 8
    assert pp_gpu == pp_ref
    assert ts_gpu == ts_ref


@need_both
def test_same_bytes_with_placed_pipes(tmp_path):
    """LSDR_ARENA_GIB: the host framework's device pipes come out of an lsdr_arena (the fastest windows of one allocation) instead of separate
    allocations — lsdr_malloc behind pipebuf's storage.  Same command line (the default front end, --resample, large pipes), same bytes."""
    from leansdr_amd import synth
    x, _ = synth.qpsk_baseband(120 * 40000, 120, seed=4, rms=1.0, snr_db=15.0, circular=False)
    flags = ["--f32", "--float-scale", "75", "-f", "240e6", "--sr", "2000e3", "--cr", "1/2", "--resample", "--fd-pp", "3", "--buf-factor", "64", "-v"]
    (ts_ref, pp_ref, _), (ts_gpu, pp_gpu, err) = _run_both(flags, x.astype(np.complex64).tobytes(), tmp_path, extra_fd=True, gpu_env={"LSDR_ARENA_GIB": "3"})
    assert "LSDR_ARENA_GIB" not in err, err[-500:]          # (the arena was there: no fallback message)
    assert len(pp_ref) > 100000 * 8 and pp_gpu == pp_ref and ts_gpu == ts_ref


@need_both
@pytest.mark.parametrize("cw,amp", [(0.0137, 0.4), (-0.0137, 0.4), (-0.0027, 0.05)], ids=["strong_out_of_band_pos", "strong_out_of_band_neg", "weak_in_band"])
def test_default_front_end_fused(tmp_path, cw, amp):
    """The DEFAULT front end (`--anf 1 --resample`) with LSDR_FUSE_NOTCH=1: the reference's unchanged leandvb.cc builds auto_notch,
    spectrum (always, leandvb.cc:335) and fir_filter as separate blocks; before the scheduler's first pass the fir_filter block finds the
    notch in front of it, switches the unread spectrum tap off and runs notch + filter as ONE block (lsdr_notch_fir: the notched 120-sps
    stream never exists).  A tolerance mode: the transport stream — a real DVB-S signal from the reference's own leantsgen | leandvbtx |
    leanchansim with a CW interferer added — is the reference binary's from this graph's first packet on, for an interferer 3x the
    signal's amplitude next to its band (the notch's job; the reference delivers 255 of the 320 packets).  With a WEAK interferer inside
    the band the reference itself delivers 94–132 of them, its lock comes and goes, and a 1e-5 perturbation of the receiver's input moves
    those moments: there only the preprocessed stream (--fd-pp) is compared.  It is within 1e-3 of full scale of the reference's
    everywhere (include/lsdr_hip.h), 2e-5 for the positive bin, 2e-6 before the first detect."""
    ref = os.path.dirname(REFBIN)
    gen = f"{ref}/leantsgen -c 320 | {ref}/leandvbtx -f 120 --power 0 --agc | {ref}/leanchansim --awgn -20 --deterministic"
    r = subprocess.run(gen, shell=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    x = np.frombuffer(r.stdout, np.complex64).copy()          # 60 M samples at 120 per symbol, RMS 0.135
    assert len(x) > 50_000_000
    x += (amp * np.exp(2j * np.pi * cw * np.arange(len(x)))).astype(np.complex64)
    flags = ["--f32", "--float-scale", "550", "-f", "240e6", "--sr", "2000e3", "--cr", "1/2", "--resample", "--fd-pp", "3", "-v"]
    (ts_ref, pp_ref, _), (ts_gpu, pp_gpu, err_gpu) = _run_both(flags, x.tobytes(), tmp_path, extra_fd=True, gpu_env={"LSDR_FUSE_NOTCH": "1"})
    assert "fused with auto_notch" in err_gpu
    a, b = np.frombuffer(pp_ref, np.complex64), np.frombuffer(pp_gpu, np.complex64)
    m = min(len(a), len(b))
    assert m > 1800000 and len(a) - m < 4096
    e = np.abs(a[:m].astype(np.complex128) - b[:m]) / np.abs(a).max()
    assert e.max() <= (2e-5 if cw > 0 else 1e-3), e.max()
    assert e[:100000].max() <= 2e-6          # (before the first detect: the plain filter)
    if amp < 0.1:
        return
    pk = lambda ts: [ts[i:i + 188] for i in range(0, len(ts) - 187, 188)]
    want, got = pk(ts_ref), pk(ts_gpu)
    assert len(want) > 200 and len(got) > 200 and got[0] in want
    i0 = want.index(got[0])
    n = min(len(got), len(want) - i0)
    assert got[:n] == want[i0:i0 + n] and len(want) - i0 - n <= 8          # the same packets from its lock on, to (nearly) the reference's last one


@pytest.mark.parametrize("size", [1024, 4099, 1 << 18])
def test_pipes_with_ends_on_both_sides(tmp_path, size):
    """tests/host/pipe_sides_test.cc: one host-written pipe read by a GPU block AND a host block, one device-written pipe read
    by a GPU block AND a host block, small pipes (constant compaction with uploads/downloads in flight): every reader sees
    every item exactly once, in order."""
    exe = tmp_path / "pipe_sides"
    host = os.path.join(ROOT, "leansdr_amd", "host")
    lib = os.path.join(ROOT, "leansdr_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-w", "-I", host, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "pipe_sides_test.cc"), "-o", str(exe), "-L", lib, "-llsdr_hip", f"-Wl,-rpath,{lib}"])
    rng = np.random.default_rng(3)
    n = 300000 + 17
    x = (rng.integers(-1000, 1000, n) + 1j * rng.integers(-1000, 1000, n)).astype(np.complex64)
    f3, f4 = tmp_path / "raw.bin", tmp_path / "x2.bin"
    r = subprocess.run(f"{exe} {size} 3>{f3} 4>{f4}", shell=True, input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    half = np.frombuffer(r.stdout, np.complex64)
    raw = np.frombuffer(f3.read_bytes(), np.complex64)
    x2 = np.frombuffer(f4.read_bytes(), np.complex64)
    assert len(raw) == len(x2) == len(half) == n
    assert np.array_equal(raw, x) and np.array_equal(x2, x * 2) and np.array_equal(half, x * np.float32(0.5))
