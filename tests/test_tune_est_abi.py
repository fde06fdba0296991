"""lsdr_tune_est without a GPU: the C ABI (header as C99, record size, exported symbols) and the estimator's float64 restatement
(tune_common.estimate) against the TRUE carrier offset of synthetic captures — what the device is then held to in test_gpu_tune_est.py.

Bounds.  |tune − offset| ≤ W/8 with W = 1/(2048·8), the tuning window of the tiled receivers at the largest supported omega (8 samples per
symbol): the tiles need the carrier inside W, an eighth of the narrowest W leaves the loops seven eighths (7.6e-6 cycles per sample).
quality ≥ 10 × what Gaussian noise alone reaches (measured here, eight blocks, 40 captures).  Measured on this code: max |tune − offset|
2.3e-6 (1.2 samples per symbol), 1.0e-6 (4), 2.0e-6 (8); quality 347 … 2071; Gaussian noise at most 3.12.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import tune_common as tc
from batch_common import shifted
from conftest import ROOT

SYMBOLS = ("lsdr_tune_est_create", "lsdr_tune_est_destroy", "lsdr_tune_est_run_async", "lsdr_tune_est_wait")


def test_header_is_c99_and_the_record_has_32_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lsdr_hip.h"\n'
                   "typedef char record_is_32_bytes[sizeof(lsdr_tune_estimate) == 32 ? 1 : -1];\n"
                   "typedef char cfg_is_32_bytes[sizeof(lsdr_tune_est_cfg) == 32 ? 1 : -1];\n"
                   "int main(void) { lsdr_tune_est_cfg c; lsdr_tune_estimate e; c.blocks = 0; e.power[2] = 0; (void)c; (void)e;\n"
                   "  int (*w)(lsdr_tune_est *, lsdr_tune_estimate *) = lsdr_tune_est_wait; (void)w;\n"
                   "  return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_estimator(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.TuneEstimate) == 32 and ctypes.sizeof(capi.TuneEstCfg) == 32
    assert capi.lib.lsdr_abi_version() == 2


@pytest.fixture(scope="module")
def noise_quality():
    q = tc.gaussian_noise_quality()
    print(f"Gaussian noise alone (std 18 and 37, eight blocks, 20 seeds each): quality at most {q:.3f}")
    assert 1.0 < q < 10.0                       # condition on the yardstick: noise has no line
    return q


def _hold(cases, noise_quality, what):
    errs, quals = [], []
    for name, f, iq in cases:
        e = tc.estimate(tc.to_complex(iq))
        errs.append(abs(e["tune"] - f)); quals.append(e["quality"])
        assert e["blocks"] == tc.BLOCKS
        assert errs[-1] <= tc.W8, f"{name} offset {f}: tune {e['tune']}, off by {errs[-1]:.3e} > {tc.W8:.3e}"
        assert e["quality"] >= 10 * noise_quality, f"{name} offset {f}: quality {e['quality']}"
    print(f"{what}: max |tune - offset| {max(errs):.3e} (bound {tc.W8:.3e}), quality {min(quals):.0f} ... {max(quals):.0f}")


def test_restatement_recovers_the_offset_at_1p2_samples_per_symbol(noise_quality):
    _hold([(f"noise {noise}", f, iq) for noise, f, iq in tc.sixteen()], noise_quality, "1.2 samples per symbol, noise 7.5 and 18")


@pytest.mark.parametrize("sps,noise", [(4, 7.5), (8, 18.0)])
def test_restatement_recovers_the_offset_at_more_samples_per_symbol(noise_quality, sps, noise):
    from leansdr_amd import synth_dvbs
    iq, _ = synth_dvbs.capture_u8(n_packets=60, sps_num=sps, sps_den=1, seed=11, noise_std=noise)
    head = np.ascontiguousarray(iq[: 2 * tc.N * tc.BLOCKS])
    assert len(head) == 2 * tc.N * tc.BLOCKS
    _hold([(f"sps {sps} noise {noise}", f, shifted(head, f) if f else head) for f in tc.OFFSETS], noise_quality, f"{sps} samples per symbol, noise {noise}")


def test_restatement_edges():
    z = tc.to_complex(tc.shifted_head(7.5, 1e-3))
    assert tc.estimate(z[: tc.N - 1]) == dict(tune=0.0, quality=0.0, bin=0, blocks=0, power=[0.0, 0.0, 0.0], mean_power=0.0)
    assert tc.estimate(z[: 3 * tc.N + 1])["blocks"] == 3 and tc.estimate(z, blocks=64)["blocks"] == 8
    zero = tc.estimate(np.zeros(2 * tc.N, np.complex128))
    assert zero["blocks"] == 2 and zero["tune"] == 0.0 and zero["quality"] == 0.0
    # the sign and the wrap of step 5
    assert tc.tune_from_peak(16, 1.0, 4.0, 1.0) == pytest.approx((16 + 1 / 3) / (4 * tc.N))
    assert tc.tune_from_peak(16, 1.0, 4.0, 0.5) == pytest.approx((16 - 1 / 3) / (4 * tc.N))
    assert tc.tune_from_peak(4095, 0.0, 4.0, 1.0) == pytest.approx((-1 + 1 / 3) / (4 * tc.N))
    assert tc.tune_from_peak(2048, 0.0, 4.0, 0.0) == -0.125
