"""lsdr_tune_track and lsdr_derotate_batch without a GPU.

a  The integer arithmetic the host and the kernel share (leansdr_amd/csrc/derotate_batch_device.h) and the tracker's frame plan and record
   (tune_track_device.h), compiled into a stand-alone program (tests/track_host.hip, its own main) under AddressSanitizer and UBSan and
   checked against Python integers (track_common): floor division with negative differences, the knot put at sample 0, extrapolation at
   both ends, Φ continuity at every knot, wrap-around of φ, one knot and no knots, and the four rules a track can break.  (The refusals
   that need an object — a misaligned pointer, n above max_samples, more than max_knots knots, a run in flight — are held on the GPU, in
   test_gpu_tune_track.py.)
b  The float64 restatement's accuracy (track_common.track) on captures whose carrier moves: capture(1000, 11, 7.5) and capture(1000, 11, 18)
   with an offset of A·sin(2πn/T + φ), T the capture's length, for A = 2e-3 with φ = 0 and 1, and A = 4e-3.  The piecewise-linear track
   through the accepted knots, its first and last slope run on to the capture's ends, stays within a quarter of the tiles' window of f[n]
   over the whole capture: the window is 1/(2048·1.2) = 4.07e-4 at 1.2 samples per symbol, the bound 1.0e-4.
"""
import os
import random
import subprocess

import numpy as np
import pytest
import track_common as trk
import tune_common as tc
from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BOUND = 1.0e-4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("track_host") / "track_host"
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                            "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "leansdr_amd", "csrc"), os.path.join(ROOT, "tests", "track_host.hip"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]

    def ask(text):
        run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
        return run.stdout.split("\n")
    return ask


def _knot_case(knots, asks):
    return f"K {len(knots)} {len(asks)}\n" + "".join(f"{s} {float(t).hex()}\n" for s, t in knots) + " ".join(str(a) for a in asks) + "\n"


def _check_knots(lines, knots, asks, name):
    """Consumes one case's answer from `lines` and compares it with the Python integers."""
    want = trk.knot_error(knots)
    rule, bad = (int(w) for w in lines.pop(0).split())
    if want:
        assert (rule, bad) == want, (name, rule, bad, want)
        return
    assert rule == 0, (name, rule, bad)
    segs = trk.segments(knots)
    assert int(lines.pop(0)) == len(segs), name
    for g in segs:
        assert tuple(int(w) for w in lines.pop(0).split()) == g, (name, g)
    for n in asks:
        si = trk.segment_of(segs, n)
        start, phi, F, S = segs[si]
        assert tuple(int(w) for w in lines.pop(0).split()) == (si, trk.phase(segs[si], n), (F + S * (n - start)) & trk.M64), (name, n)
    # Φ is continuous at every knot: the segment in front, run on to the knot, gives the knot's own Φ
    for a, b in zip(segs, segs[1:]):
        assert trk.phase(a, b[0]) == b[1], name


def test_knot_arithmetic_against_python_integers(program):
    rng = random.Random(7)
    top = (1 << 31) - 1
    cases = [("no knots", [], [0, 1, 12345, top]),
             ("one knot in the middle", [(1000, 1e-3)], [0, 999, 1000, 1001, 1 << 30]),
             ("one knot on sample 0", [(0, -0.25)], [0, 1, 4097]),
             ("a rising and a falling segment, knots only in the middle", [(1000, -1e-3), (5000, 2e-3), (9001, -3e-3)], [0, 1, 999, 1000, 4999, 5000, 5001, 9000, 9001, 20000]),
             ("a difference the distance does not divide, negative", [(3, 1e-3), (10, 1e-3 - 7.5 * 2.0 ** -60)], [0, 2, 3, 9, 10, 11]),
             ("a knot on sample 0 and one on the last", [(0, 0.1), (top, -0.1)], [0, 1, top - 1, top]),
             ("the phase wraps many times", [(0, 0.4999), (7, -0.4999 + 0.5 - 2.0 ** -40), (1 << 20, 0.3)], [0, 6, 7, 8, 1 << 19, 1 << 20, 1 << 30]),
             ("tiny tunes that are no whole frequency words, ties included", [(5, 2.0 ** -65), (6, -1.5 * 2.0 ** -64), (7, 2.5 * 2.0 ** -64), (9, 2.0 ** -70 * 3)], [0, 5, 6, 7, 9, 100]),
             ("neighbouring samples", [(0, 0.01), (1, 0.02), (2, 0.01), (3, 0.3)], [0, 1, 2, 3, 4]),
             ("31 knots", [(100 + 37 * i * i, 0.12 * np.sin(i)) for i in range(31)], list(range(0, 40000, 997))),
             # the rules
             ("sample 2^31", [(5, 0.0), (1 << 31, 0.0)], []), ("descending", [(5, 0.0), (9, 0.0), (8, 0.0)], []), ("twice the same", [(5, 0.0), (5, 0.1)], []),
             ("tune 0.5", [(1, 0.5)], []), ("tune -0.5", [(1, 0.1), (2, -0.5)], []), ("tune nan", [(1, float("nan"))], []),
             ("tune inf", [(0, 0.0), (1, float("inf"))], []), ("a step of 0.5", [(0, 0.25), (10, -0.25)], []), ("a step above 0.5", [(0, 0.3), (10, -0.3)], []),
             ("a step just under 0.5", [(0, 0.25), (10, -0.25 + 2.0 ** -40)], [0, 5, 10, 11])]
    for i in range(40):
        k = rng.randint(1, 12)
        samples = sorted(rng.sample(range(0, 1 << rng.choice([4, 12, 24, 31])), k))
        tunes = [rng.uniform(-0.24, 0.24) for _ in range(k)]
        cases.append((f"random {i}", list(zip(samples, tunes)), [0] + [rng.randrange(0, 1 << 31) for _ in range(8)] + samples + [s + 1 for s in samples]))
    lines = program("".join(_knot_case(k, a) for _, k, a in cases))
    for name, knots, asks in cases:
        _check_knots(lines, knots, asks, name)
    assert [l for l in lines if l.strip()] == []
    assert sum(1 for _, k, _ in cases if trk.knot_error(k)) == 9
    # floor, not truncation: a negative difference that the distance does not divide
    segs = trk.segments(cases[4][1])
    dF = trk.freq_word(cases[4][1][1][1]) - trk.freq_word(cases[4][1][0][1])
    assert dF < 0 and dF % 7 != 0 and segs[1][3] == (dF // 7) & trk.M64 and (dF // 7) != int(dF / 7)
    # the knot at sample 0: the first slope run back, so that the frequency at the first knot is the knot's
    g0, g1 = trk.segments(cases[3][1])[:2]
    assert g0[0] == 0 and g0[1] == 0 and (g0[2] + g0[3] * 1000) & trk.M64 == g1[2] and g0[3] == g1[3]


def test_frame_plan_and_record(program):
    asks = [(n, b, h) for b, h in ((4, 16), (1, 1), (16, 3), (4, 4)) for n in (0, 1, b * 4096 - 1, b * 4096, b * 4096 + 1, b * 4096 + 4095, b * 4096 + 4096,
                                                                                 (b + h) * 4096 - 1, (b + h) * 4096, (b + h) * 4096 + 4096, 1958423, 8 << 20, (8 << 20) + 5000)]
    recs = [(8192, 17, 1.0, 4.0, 0.5, 40.0, 4, 30.0), (8192, 4095, 0.0, 4.0, 1.0, 4096.0 * 4.0 / 30.0, 4, 30.0), (0, 0, 0.0, 0.0, 0.0, 0.0, 4, 30.0),
            (1 << 40, 2048, 0.0, 4.0, 0.0, 4096.0, 16, 4.0), (5, 5, 1.0, 2.0, 1.0, 8192.0, 1, 1.0)]
    text = "".join(f"F {n} {b} {h}\n" for n, b, h in asks)
    text += "".join(f"R {c} {k} {float(l).hex()} {float(p).hex()} {float(r).hex()} {float(s).hex()} {b} {float(q).hex()}\n" for c, k, l, p, r, s, b, q in recs)
    lines = program(text)
    for n, b, h in asks:
        want = trk.frame_starts(n, b, h * 4096)
        assert int(lines.pop(0)) == len(want), (n, b, h)
        assert [int(w) * 4096 for w in lines.pop(0).split()] == want, (n, b, h)
    for c, k, l, p, r, s, b, q in recs:
        held, bin_, tune, quality, mean = lines.pop(0).split()
        mean_w = np.float32(s) * (np.float32(1.0) / np.float32(4096.0))
        quality_w = np.float32(p) / mean_w if p > 0 else np.float32(0.0)
        assert int(bin_) == k and float.fromhex(mean) == float(mean_w) and float.fromhex(quality) == float(quality_w)
        assert float.fromhex(tune) == float(np.float32(tc.tune_from_peak(k, l, p, r)))
        assert int(held) == (0 if quality_w >= np.float32(q) else 1)
    assert [int(r_) for r_ in ([trk.frame_starts(1958423, 4, 65536)[-1], len(trk.frame_starts(1958423, 4, 65536))])] == [1941504, 31]


def test_restatement_edges():
    z = tc.to_complex(tc.shifted_head(7.5, 1e-3, 9))
    none = trk.track(z[: 4 * trk.N - 1])
    assert none["frames"] == [] and none["accepted"] == 0 and none["tune_first"] == 0.0 and none["quality_min"] == 0.0
    one = trk.track(z[: 4 * trk.N])
    assert len(one["frames"]) == 1 and one["frames"][0]["center"] == 2 * trk.N
    e = tc.estimate(z, 4)
    assert {k: one["frames"][0][k] for k in ("tune", "quality", "bin", "power", "mean_power")} == {k: e[k] for k in ("tune", "quality", "bin", "power", "mean_power")}
    two = trk.track(z[: 9 * trk.N], hop=4096 * 5)                  # frames at 0 and at 5 blocks: the end frame is the hop frame, once
    assert [f["center"] for f in two["frames"]] == [2 * trk.N, 7 * trk.N]
    three = trk.track(z[: 9 * trk.N], hop=4096 * 4)                 # frames at 0, 4 and the end frame at 5
    assert [f["center"] for f in three["frames"]] == [2 * trk.N, 6 * trk.N, 7 * trk.N]
    assert trk.track_value([], 3).tolist() == [0, 0, 0] and trk.track_value([(5, 0.25)], 2).tolist() == [0.25, 0.25]
    assert trk.track_value([(1, 1.0), (3, 2.0)], 6).tolist() == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]


@pytest.mark.parametrize("noise", [7.5, 18.0])
@pytest.mark.parametrize("A,phase", [(2e-3, 0.0), (2e-3, 1.0), (4e-3, 0.0)])
def test_restatement_follows_the_drift(noise, A, phase):
    iq, f = trk.drifted_capture(noise, A, phase)
    n = len(f)
    t = trk.track(tc.to_complex(iq))
    knots = trk.knots_of(t["frames"])
    err = float(np.max(np.abs(trk.track_value(knots, n) - f)))
    inside = float(np.mean(np.abs(f - t["tune_first"]) <= trk.WINDOW))
    print(f"noise {noise} A {A} phase {phase}: {len(t['frames'])} frames, {t['accepted']} accepted, track error {err:.2e} (bound {BOUND:.1e}), "
          f"quality at least {t['quality_min']:.0f}; {100 * inside:.0f} % of the capture inside the window around the first frame's tune")
    assert len(t["frames"]) == 31 and t["frames"][-1]["center"] == (n - 4 * trk.N) // trk.N * trk.N + 2 * trk.N
    assert err <= BOUND, err
    assert t["accepted"] == len(t["frames"]) and t["quality_min"] >= 30.0
    # the end frame and the extrapolation are part of the definition: without them the ends are off by more than the bound
    flat = np.interp(np.arange(n), [k[0] for k in knots[:-1]], [k[1] for k in knots[:-1]])
    assert np.max(np.abs(flat - f)) > BOUND
