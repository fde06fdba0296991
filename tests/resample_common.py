"""Shared helpers of the resample batch's tests (lsdr_resample_batch, include/lsdr_hip.h): its arithmetic restated in numpy float32 — a test
oracle, never imported by the product — leandvb's filter design rule in numpy, and the synthetic oversampled captures.

The arithmetic (the header states it the same way), every operation one float32 rounding.  For a capture of n items, N taps h, decimation D:
  1 x[k] = float(item − Z)·in_scale (no multiply for a scale of 0 or 1);
  2 ifreq = (int)(tune·65536), C truncation; phase index of sample k: (−k·ifreq) mod 65536 in [0, 65536);
    (c, s) = T[index], T[j] = ((float)cos(2πj/65536), (float)sin(2πj/65536)) evaluated in double;
    y.re = x.re·c − x.im·s;  y.im = x.re·s + x.im·c;
  3 out[m] = Σ_{i=0…N−1} h[i]·y[N + m·D − i], i ascending, re and im separately, each from 0 by acc = acc + h[i]·y;
  4 produced = n ≥ N ? min((n − N)//D, cap_out) : 0; consumed = produced·D.
"""
import functools

import numpy as np
from batch_common import shifted

F32 = np.float32
# the restatement against the reference chain rotator -> fir_filter: four times the largest deviation measured in test_resample_abi.py (its
# docstring has the figures), rounded up to one digit; on the first CHAIN_SAMPLES samples of the 12-sps capture at CHAIN_TUNES
REF_CHAIN_BOUND = 4e-2
CHAIN_TUNES = (0.01, -0.03, 0.1, -0.12)
CHAIN_SAMPLES = 40000
Z = {"cu8": 128, "cs8": 0, "cu16": 32768, "cs16": 0}


@functools.lru_cache(maxsize=None)
def table():
    """T: (cos, sin) of 2πj/65536, evaluated in float64, rounded to float32."""
    a = 2.0 * np.pi * np.arange(65536, dtype=np.float64) / 65536.0
    return np.cos(a).astype(F32), np.sin(a).astype(F32)


def convert(items, fmt="cu8", scale=0.0):
    """Step 1: (re, im) float32 arrays of interleaved items."""
    a = np.asarray(items).reshape(-1, 2)
    if fmt == "cf32":
        x = a.astype(F32)
    else:
        x = (a.astype(np.int64) - Z[fmt]).astype(F32)
    if scale not in (0.0, 1.0):
        x = x * F32(scale)
    return np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])


def ifreq_of(tune):
    """(int)(tune·65536) as C computes it: the product in float32, truncated towards zero."""
    return int(F32(tune) * F32(65536))


def rotate(re, im, ifreq):
    """Step 2."""
    k = np.arange(len(re), dtype=np.int64)
    idx = (-k * int(ifreq)) % 65536
    c, s = table()
    c, s = c[idx], s[idx]
    return re * c - im * s, re * s + im * c


def fir(re, im, h, D, cap_out=None):
    """Steps 3 and 4 on the rotated stream: (complex64 outputs, consumed)."""
    h = np.asarray(h, F32)
    N, n = len(h), len(re)
    produced = (n - N) // D if n >= N else 0
    if cap_out is not None:
        produced = min(produced, cap_out)
    accr, acci = np.zeros(produced, F32), np.zeros(produced, F32)
    if produced:
        base = N + np.arange(produced, dtype=np.int64) * D
        for i in range(N):
            accr = accr + h[i] * re[base - i]
            acci = acci + h[i] * im[base - i]
    out = np.empty(produced, np.complex64)
    out.real, out.imag = accr, acci
    return out, produced * D


def resample(items, tune, h, D, fmt="cu8", scale=0.0, cap_out=None):
    """The whole restatement: (complex64 outputs, consumed, ifreq)."""
    re, im = convert(items, fmt, scale)
    f = ifreq_of(tune)
    yr, yi = rotate(re, im, f)
    out, consumed = fir(yr, yi, h, D, cap_out)
    return out, consumed, f


def design(omega, rolloff=0.35, rej=10.0, decim=0):
    """leandvb.cc:353-378 with Fm = 1 and Fs = omega, in float32 like the reference's floats: (decim, order, Fcut)."""
    omega, rolloff, rej = F32(omega), F32(rolloff), F32(rej)
    d = int(decim) if decim else max(1, int(omega / F32(4)))
    transition = F32(0.5) * rolloff
    order = int(rej * omega / (F32(22) * transition))
    order = ((order + 1) // 2) * 2
    fcut = F32(0.5) * (F32(1) + rolloff / F32(2)) / omega
    return d, order, F32(fcut)


def same_values(a, b):
    """Equal as values: bit for bit but for the sign of a zero."""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    return a.shape == b.shape and bool(np.all(a.view(F32) == b.view(F32)))


@functools.lru_cache(maxsize=None)
def capture_sps(n_packets, sps, noise):
    """A cu8 capture at `sps` samples per symbol (seed 11): (IQ items, the set of transmitted packets)."""
    from leansdr_amd import synth_dvbs
    iq, ts = synth_dvbs.capture_u8(n_packets=n_packets, sps_num=sps, sps_den=1, seed=11, noise_std=noise)
    return np.ascontiguousarray(iq), {bytes(p) for p in np.asarray(ts, np.uint8).reshape(-1, 188)}


@functools.lru_cache(maxsize=None)
def shifted_sps(n_packets, sps, noise, f, n_samples=None):
    """capture_sps shifted by f cycles per sample (its first n_samples items; None: all)."""
    iq = capture_sps(n_packets, sps, noise)[0]
    if n_samples is not None:
        iq = iq[: 2 * n_samples]
    return np.ascontiguousarray(shifted(iq, f) if f else iq)


def formats_of(u8):
    """[(name, items, capi format name, in_scale)]: the cu8 items as the four other formats that convert to the same floats."""
    s8 = (u8.astype(np.int16) - 128).astype(np.int8)
    s16 = (s8.astype(np.int16) * 256).astype(np.int16)
    u16 = (s16.astype(np.int32) + 32768).astype(np.uint16)
    f32 = s8.astype(np.float32)
    return [("cs8", s8, "IN_CS8", 0.0), ("cu16", u16, "IN_CU16", 2.0 ** -8), ("cs16", s16, "IN_CS16", 2.0 ** -8), ("cf32", f32, "IN_CF32", 1.0)]
