"""Shared helpers of the carrier-offset estimator's tests (lsdr_tune_est, include/lsdr_hip.h): the estimator restated in float64 numpy — a
test oracle, never imported by the product — the sample formats' conversion, and the captures the CPU and the GPU tests share.

The estimator (the header states it the same way).  For one capture of n items, M = min(blocks, n // 4096) whole blocks of N = 4096 samples
from the capture's first sample:
  1 convert: float(item − Z)·in_scale;  2 divide every block by its own RMS (an all-zero block contributes zeros);
  3 w = z⁴, X = FFT_N(w), rectangular window;  4 P[k] = Σ_blocks |X[k]|², in block order;
  5 k0 = first arg-max of P, c = P[k0], l and r its cyclic neighbours, m = sqrt(max(l, r)/c), δ = ±m/(1 + m) (+ when r ≥ l),
    κ = k0 + δ taken into [−N/2, N/2), tune = κ/(4N) cycles per sample;  6 a capture multiplied by exp(+j2π·f·n) yields +f;
  7 quality = c / mean(P);  8 M == 0: the record is all zeros.
"""
import functools

import numpy as np
from batch_common import capture, shifted

N = 4096
W8 = 1.0 / (2048 * 8) / 8          # an eighth of the tuning window at the largest supported omega (8 samples per symbol): 7.6e-6
OFFSETS = [0.0, 1e-3, -1e-3, 3e-3, 0.02, -0.05, 0.1, -0.12]
NOISES = [7.5, 18.0]
BLOCKS = 8


def to_complex(items, fmt="cu8", scale=1.0):
    """The items of a capture (interleaved I, Q) as complex128: float(item − Z)·scale, like the device's loads."""
    a = np.asarray(items).reshape(-1, 2).astype(np.float64)
    z = {"cu8": 128.0, "cs8": 0.0, "cu16": 32768.0, "cs16": 0.0, "cf32": 0.0}[fmt]
    return ((a[:, 0] - z) + 1j * (a[:, 1] - z)) * (scale if scale else 1.0)


def tune_from_peak(k0, l, c, r):
    """Step 5 in float64: the tune for the peak bin k0 with powers l, c, r."""
    if not c > 0:
        return 0.0
    m = np.sqrt(max(l, r) / c)
    d = m / (1.0 + m)
    kappa = k0 + (d if r >= l else -d)
    if kappa >= N / 2:
        kappa -= N
    return kappa / (4.0 * N)


def estimate(z, blocks=BLOCKS):
    """The estimator on the complex samples z: dict(tune, quality, bin, blocks, power [l, c, r], mean_power)."""
    z = np.asarray(z, np.complex128)
    M = min(int(blocks), len(z) // N)
    if M == 0:
        return dict(tune=0.0, quality=0.0, bin=0, blocks=0, power=[0.0, 0.0, 0.0], mean_power=0.0)
    P = np.zeros(N)
    for b in range(M):
        zb = z[b * N:(b + 1) * N]
        rms = np.sqrt(np.mean(np.abs(zb) ** 2))
        zb = zb / rms if rms > 0 else np.zeros(N, np.complex128)
        z2 = zb * zb
        P += np.abs(np.fft.fft(z2 * z2)) ** 2
    k0 = int(np.argmax(P))
    l, c, r = float(P[(k0 - 1) % N]), float(P[k0]), float(P[(k0 + 1) % N])
    mean = float(P.mean())
    return dict(tune=tune_from_peak(k0, l, c, r), quality=c / mean if c > 0 else 0.0, bin=k0, blocks=M, power=[l, c, r], mean_power=mean)


@functools.lru_cache(maxsize=None)
def shifted_head(noise, f, n_blocks=BLOCKS):
    """The first n_blocks blocks of capture(1000, 11, noise) shifted by f cycles per sample (cu8 items)."""
    iq = capture(1000, 11, noise)[0][: 2 * N * n_blocks]
    return np.ascontiguousarray(shifted(iq, f) if f else iq)


def sixteen():
    """[(noise, offset, cu8 items)]: the 16 shifted eight-block captures of the accuracy tests."""
    return [(noise, f, shifted_head(noise, f)) for noise in NOISES for f in OFFSETS]


def gaussian_noise_quality(stds=(18.0, 37.0), seeds=20, blocks=BLOCKS):
    """The largest quality of Gaussian-noise-only cu8 captures (no carrier): what `quality` reads when there is nothing to find."""
    worst = 0.0
    for std in stds:
        for seed in range(seeds):
            rng = np.random.default_rng(1000 + seed)
            x = np.clip(np.rint(rng.normal(0.0, std, 2 * N * blocks) + 128), 0, 255).astype(np.uint8)
            worst = max(worst, estimate(to_complex(x), blocks)["quality"])
    return worst
