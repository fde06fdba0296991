"""Shared helpers of the symbol-rate estimator's tests (lsdr_rate_est, include/lsdr_hip.h): the estimator restated in float64 numpy — a
test oracle, never imported by the product — the captures the CPU and the GPU tests share, and what Gaussian noise alone reads.

The estimator (the header states it the same way).  For one capture of n items, M = min(blocks, n // 4096) whole blocks of N = 4096 samples
from the capture's first sample:
  1 convert: float(item − Z)·in_scale;
  2 per block s = mean |z|², p[n] = |z[n]|²/s − 1; a block with s = 0 contributes zeros to every sum and is not counted in M₁;
  3 X = FFT_N(p + 0j), rectangular window; P[k] += |X[k]|², in block order;
  4 c₁ += Σ_{n=1…N−1} z[n]·conj(z[n−1]) / s; R = |c₁| / (M₁·(N − 1)), M₁ the number of nonzero blocks;
  5 bins k ∈ [k_lo, N/2], k_lo = max(2, ⌊N/omega_max⌋) (with omega_max < 2: max(2, ⌊N·(1 − 1/omega_min)⌋)); floor = mean of P over them; k0 = first arg-max, c = P[k0];
    l′ = max(P[k0−1] − floor, 0), r′ = max(P[k0+1] − floor, 0) (P is symmetric: P[N/2+1] = P[N/2−1]); m = sqrt(max(l′, r′)/c),
    δ = ±m/(1 + m), + when r′ ≥ l′; line = (k0 + δ)/N, and 1 − line where that exceeds 0.5;
  6 candidates omega_a = 1/line (≥ 2) and omega_b = 1/(1 − line) (in [1, 2]); one outside [omega_min, omega_max] is dropped; with both, a
    when |R − |sinc(line)|| < |R − |sinc(1 − line)||, else b; `other` is the one not chosen (0: dropped); ambiguous = both admissible and
    line > 0.4;
  7 quality = c / floor;  8 M == 0, c == 0 or no admissible candidate: the record is all zeros.
"""
import functools
import math

import numpy as np
from batch_common import shifted

N = 4096
BLOCKS = 64
OMEGA_MIN, OMEGA_MAX = 1.016, 64.0
SHIFT = 0.03                       # cycles per sample: every capture of the case list is off tune by this much
SPS = [(6, 5), (3, 2), (3, 1), (4, 1), (8, 1), (12, 1)]
NOISES = [7.5, 18.0]
REL = 2.5e-4                       # a quarter of the 1e-3 by which the reference's --sr may be off with its TS unchanged
ZERO = dict(omega=0.0, other=0.0, line=0.0, quality=0.0, corr=0.0, bin=0, blocks=0, ambiguous=0, power=[0.0, 0.0, 0.0], floor=0.0)


def to_complex(items, fmt="cu8", scale=1.0):
    """The items of a capture (interleaved I, Q) as complex128: float(item − Z)·scale, like the device's loads."""
    a = np.asarray(items).reshape(-1, 2).astype(np.float64)
    z = {"cu8": 128.0, "cs8": 0.0, "cu16": 32768.0, "cs16": 0.0, "cf32": 0.0}[fmt]
    return ((a[:, 0] - z) + 1j * (a[:, 1] - z)) * (scale if scale else 1.0)


def k_lo(omega_min=OMEGA_MIN, omega_max=OMEGA_MAX):
    lo, hi = float(np.float32(omega_min)), float(np.float32(omega_max))
    return max(2, int(math.floor(N * (1.0 - 1.0 / lo if hi < 2 else 1.0 / hi))))


def from_peak(k0, l, c, r, floor, corr, omega_min=OMEGA_MIN, omega_max=OMEGA_MAX):
    """Steps 5 and 6 in float64 from the peak bin, its powers, the floor and R: dict(omega, other, line, ambiguous), or None where the
    record is all zeros."""
    if not c > 0:
        return None
    lo, hi = float(np.float32(omega_min)), float(np.float32(omega_max))
    lp, rp = max(l - floor, 0.0), max(r - floor, 0.0)
    m = math.sqrt(max(lp, rp) / c)
    d = m / (1.0 + m)
    line = (k0 + (d if rp >= lp else -d)) / N
    if line > 0.5:
        line = 1.0 - line
    a, b = 1.0 / line, 1.0 / (1.0 - line)
    ok_a, ok_b = lo <= a <= hi, lo <= b <= hi
    if not (ok_a or ok_b):
        return None
    if ok_a and ok_b:
        pick_a = abs(corr - abs(np.sinc(line))) < abs(corr - abs(np.sinc(1.0 - line)))
    else:
        pick_a = ok_a
    omega, other = (a, b if ok_b else 0.0) if pick_a else (b, a if ok_a else 0.0)
    return dict(omega=omega, other=other, line=line, ambiguous=int(ok_a and ok_b and line > 0.4))


def estimate(z, blocks=BLOCKS, omega_min=OMEGA_MIN, omega_max=OMEGA_MAX):
    """The estimator on the complex samples z: dict(omega, other, line, quality, corr, bin, blocks, ambiguous, power [l, c, r], floor)."""
    z = np.asarray(z, np.complex128)
    M = min(int(blocks), len(z) // N)
    if M == 0:
        return dict(ZERO, power=[0.0, 0.0, 0.0])
    P = np.zeros(N)
    c1, M1 = 0j, 0
    for b in range(M):
        zb = z[b * N:(b + 1) * N]
        mag = np.abs(zb) ** 2
        s = mag.mean()
        if not s > 0:
            continue
        M1 += 1
        P += np.abs(np.fft.fft(mag / s - 1.0)) ** 2
        c1 += np.sum(zb[1:] * np.conj(zb[:-1])) / s
    lo = k_lo(omega_min, omega_max)
    floor = float(P[lo:N // 2 + 1].mean())
    k0 = lo + int(np.argmax(P[lo:N // 2 + 1]))
    l, c, r = float(P[k0 - 1]), float(P[k0]), float(P[k0 + 1])          # (k0 + 1 ≤ N/2 + 1: the full spectrum holds its mirror)
    corr = abs(c1) / (M1 * (N - 1)) if M1 else 0.0
    pk = from_peak(k0, l, c, r, floor, corr, omega_min, omega_max)
    if pk is None:
        return dict(ZERO, power=[0.0, 0.0, 0.0])
    return dict(pk, quality=c / floor, corr=corr, bin=k0, blocks=M, power=[l, c, r], floor=floor)


def chose_a(e):
    """Whether a record's omega is its candidate a = 1/line (otherwise b = 1/(1 − line))."""
    return abs(e["omega"] * e["line"] - 1.0) < abs(e["omega"] * (1.0 - e["line"]) - 1.0)


@functools.lru_cache(maxsize=None)
def shifted_capture(num, den, noise, n_blocks=BLOCKS, seed=11):
    """cu8 items: the first n_blocks blocks of synth_dvbs.capture_u8 at num/den samples per symbol — just enough packets for them (1632
    symbols each) — multiplied by exp(+j2π·SHIFT·n)."""
    from leansdr_amd import synth_dvbs
    n_packets = -(-n_blocks * N * den // (1632 * num)) + 1
    iq, _ = synth_dvbs.capture_u8(n_packets=n_packets, sps_num=num, sps_den=den, seed=seed, noise_std=noise)
    assert len(iq) >= 2 * N * n_blocks, (num, den, n_packets, len(iq))
    return np.ascontiguousarray(shifted(np.ascontiguousarray(iq[: 2 * N * n_blocks]), SHIFT))


def cases():
    """[(name, true omega, cu8 items)]: the twelve shifted 64-block captures of the accuracy tests."""
    return [(f"sps {num}/{den} noise {noise}", num / den, shifted_capture(num, den, noise)) for num, den in SPS for noise in NOISES]


@functools.lru_cache(maxsize=None)
def gaussian_noise_quality(stds=(18.0, 37.0), seeds=10, blocks=BLOCKS):
    """The largest quality of Gaussian-noise-only cu8 captures (no carrier): what `quality` reads when there is nothing to find."""
    worst = 0.0
    for std in stds:
        for seed in range(seeds):
            rng = np.random.default_rng(1000 + seed)
            x = np.clip(np.rint(rng.normal(0.0, std, 2 * N * blocks) + 128), 0, 255).astype(np.uint8)
            worst = max(worst, estimate(to_complex(x), blocks)["quality"])
    return worst
