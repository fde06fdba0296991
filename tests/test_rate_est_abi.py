"""lsdr_rate_est without a GPU: the C ABI (header as C99, record size, exported symbols), the estimator's float64 restatement
(rate_common.estimate) against the TRUE samples per symbol of synthetic captures — what the device is then held to in
test_gpu_rate_est.py — and capi.group_by_omega.

Bounds.  |omega/true − 1| ≤ 2.5e-4 (rate_common.REL): a quarter of the 1e-3 by which the reference's --sr may be off with its TS unchanged.
quality ≥ 8 × what Gaussian noise alone reaches (measured here with 16 and with 64 blocks, 20 captures each; the larger of the two).
Measured on this code, 64 blocks, 6/5 … 12 samples per symbol, noise 7.5 and 18, every capture 0.03 cycles per sample off tune:
max |omega/true − 1| 3.0e-5 (8 samples per symbol, where the line sits on a bin), quality 47 … 187; Gaussian noise at most 2.30 (16
blocks), 1.56 (64 blocks).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import rate_common as rc
from conftest import ROOT

SYMBOLS = ("lsdr_rate_est_create", "lsdr_rate_est_destroy", "lsdr_rate_est_run_async", "lsdr_rate_est_wait")


def test_header_is_c99_and_the_record_has_48_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lsdr_hip.h"\n'
                   "typedef char record_is_48_bytes[sizeof(lsdr_rate_estimate) == 48 ? 1 : -1];\n"
                   "typedef char cfg_is_32_bytes[sizeof(lsdr_rate_est_cfg) == 32 ? 1 : -1];\n"
                   "int main(void) { lsdr_rate_est_cfg c; lsdr_rate_estimate e; c.omega_max = 0; e.power[2] = 0; e.floor = 0; (void)c; (void)e;\n"
                   "  int (*w)(lsdr_rate_est *, lsdr_rate_estimate *) = lsdr_rate_est_wait; (void)w;\n"
                   "  return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_estimator(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.RateEstimate) == 48 and ctypes.sizeof(capi.RateEstCfg) == 32
    assert capi.lib.lsdr_abi_version() == 2


@pytest.fixture(scope="module")
def noise_quality():
    q16, q64 = rc.gaussian_noise_quality(blocks=16), rc.gaussian_noise_quality(blocks=64)
    print(f"Gaussian noise alone (std 18 and 37, 10 seeds each): quality at most {q16:.3f} with 16 blocks, {q64:.3f} with 64")
    assert 1.0 < q64 <= q16 < 5.0               # condition on the yardstick: noise has no line
    return max(q16, q64)


def test_restatement_recovers_the_rate(noise_quality):
    errs, quals = [], []
    for name, omega, iq in rc.cases():
        e = rc.estimate(rc.to_complex(iq))
        errs.append(abs(e["omega"] / omega - 1.0)); quals.append(e["quality"])
        assert e["blocks"] == rc.BLOCKS and e["ambiguous"] == 0, (name, e)
        assert rc.chose_a(e) == (omega >= 2), f"{name}: the wrong candidate, {e}"
        assert errs[-1] <= rc.REL, f"{name}: omega {e['omega']}, off by {errs[-1]:.3e} > {rc.REL:.1e}"
        assert e["quality"] >= 8 * noise_quality, f"{name}: quality {e['quality']}"
        assert e["other"] == pytest.approx(1.0 / (1.0 - 1.0 / e["omega"]), rel=1e-9)
    print(f"max |omega/true - 1| {max(errs):.3e} (bound {rc.REL:.1e}), quality {min(quals):.1f} ... {max(quals):.1f}")


def test_nine_quarters_at_noise_30_is_flagged():
    e = rc.estimate(rc.to_complex(rc.shifted_capture(9, 4, 30.0)))
    assert e["ambiguous"] == 1 and e["blocks"] == rc.BLOCKS, e
    assert min(abs(e["omega"] / 2.25 - 1), abs(e["other"] / 2.25 - 1)) <= rc.REL, e      # one of the two is the rate; which, R cannot say here
    print(f"9/4 at noise 30: omega {e['omega']:.5f}, other {e['other']:.5f}, corr {e['corr']:.3f}, quality {e['quality']:.1f}")


def test_restatement_edges():
    iq = rc.shifted_capture(6, 5, 7.5)
    z = rc.to_complex(iq)
    assert rc.estimate(z[: rc.N - 1]) == rc.ZERO and rc.estimate(z[:0]) == rc.ZERO                       # M = 0
    assert rc.estimate(z[: 3 * rc.N + 1])["blocks"] == 3 and rc.estimate(z, blocks=256)["blocks"] == 64
    assert rc.estimate(np.zeros(2 * rc.N, np.complex128)) == rc.ZERO                                      # c = 0
    # an all-zero block contributes nothing and is not counted: the record of the blocks around it
    holed = z[: 3 * rc.N].copy()
    holed[rc.N: 2 * rc.N] = 0
    h, w = rc.estimate(holed), rc.estimate(np.concatenate([z[: rc.N], z[2 * rc.N: 3 * rc.N]]))
    assert h["blocks"] == 3 and w["blocks"] == 2
    assert h["bin"] == w["bin"] and h["power"] == w["power"] and h["corr"] == pytest.approx(w["corr"], rel=1e-12) and h["omega"] == w["omega"]
    # the admissible range: 6/5 and 6 share the line at 1/6
    both = rc.estimate(z)
    assert both["omega"] == pytest.approx(1.2, rel=rc.REL) and both["other"] == pytest.approx(6.0, rel=5 * rc.REL)
    only_a = rc.estimate(z, omega_min=2.5)
    assert only_a["omega"] == pytest.approx(6.0, rel=5 * rc.REL) and only_a["other"] == 0.0 and only_a["ambiguous"] == 0
    only_b = rc.estimate(z, omega_max=1.9)
    assert only_b["omega"] == pytest.approx(1.2, rel=rc.REL) and only_b["other"] == 0.0 and only_b["bin"] == both["bin"]
    assert rc.estimate(z, omega_min=7.0, omega_max=8.0) == rc.ZERO                                        # no admissible candidate
    assert rc.estimate(z, omega_max=4.0)["bin"] >= 1024 > both["bin"]                                    # k_lo behind the line: not found
    assert rc.k_lo() == 64 and rc.k_lo(1.016, 8.0) == 512 and rc.k_lo(1.1, 1.9) == 372
    # the sign and the fold of step 5, the choice of step 6
    assert rc.from_peak(1024, 1.0, 5.0, 2.0, 1.0, 0.9)["line"] == pytest.approx((1024 + 1 / (1 + np.sqrt(5.0))) / rc.N)
    assert rc.from_peak(1024, 2.0, 5.0, 1.0, 1.0, 0.9)["line"] == pytest.approx((1024 - 1 / (1 + np.sqrt(5.0))) / rc.N)
    assert rc.from_peak(2048, 2.0, 5.0, 2.0, 1.0, 0.6)["line"] == pytest.approx(0.5 - 1 / (1 + np.sqrt(5.0)) / rc.N)
    assert rc.from_peak(1024, 0.5, 5.0, 0.5, 1.0, 0.9) == dict(omega=4.0, other=4.0 / 3.0, line=0.25, ambiguous=0)
    assert rc.from_peak(1024, 0.5, 5.0, 0.5, 1.0, 0.3) == dict(omega=4.0 / 3.0, other=4.0, line=0.25, ambiguous=0)
    assert rc.from_peak(1024, 0.5, 0.0, 0.5, 1.0, 0.3) is None and rc.from_peak(1024, 0.5, 5.0, 0.5, 1.0, 0.3, 5.0, 8.0) is None
    assert rc.from_peak(1800, 0.5, 5.0, 0.5, 1.0, 0.6)["ambiguous"] == 1 and rc.from_peak(1800, 0.5, 5.0, 0.5, 1.0, 0.6, 2.0)["ambiguous"] == 0


def test_group_by_omega(capi):
    rec = lambda omega, quality=50.0, ambiguous=0: dict(omega=omega, quality=quality, ambiguous=ambiguous)
    est = [rec(3.0001), rec(1.2), rec(3.0), rec(0.0, 0.0), rec(1.2004), rec(2.2, 40.0, 1), rec(2.9999), rec(8.0, 5.0), rec(1.2022)]
    groups, left = capi.group_by_omega(est)
    assert left == [3, 5, 7]
    assert [g[1] for g in groups] == [[1, 4], [8], [0, 2, 6]]
    assert groups[0][0] == pytest.approx(1.2002) and groups[1][0] == 1.2022 and groups[2][0] == 3.0
    assert capi.group_by_omega(est, rtol=1e-2)[0][0][1] == [1, 4, 8]
    assert capi.group_by_omega(est, min_quality=1.0)[1] == [3, 5]
    assert capi.group_by_omega([]) == ([], [])
    assert capi.RATE_MIN_QUALITY == 10.0
