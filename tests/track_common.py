"""Shared helpers of the carrier tracker's and the batch derotator's tests (lsdr_tune_track, lsdr_derotate_batch, include/lsdr_hip.h): the
tracker restated in float64 numpy on top of tune_common.estimate, the knot table restated in Python integers and the derotator in numpy
uint64 / float32 — test oracles, never imported by the product — and the captures whose carrier moves.

The tracker (the header states it the same way), N = 4096:
  frames   frame k starts at k·hop for every k with k·hop + blocks·N ≤ n; if e = ((n − blocks·N) // N)·N lies behind the last of them, one
           more frame starts at e; n < blocks·N: none;
  spectrum tune_common.estimate's steps 1 to 4 on the frame's blocks;
  peak     the first arg-max over all bins for frame 0 and for every frame with no accepted frame in front of it (and for every frame with
           span = 0); else the first maximum over the bins b − span … b + span (mod N) in that order, b the last accepted frame's bin;
           l, c, r, the interpolation and quality = c / mean(P) as in tune_common;
  accept   quality ≥ min_quality; any other frame is held: recorded, no knot, b stays.
The derotator: F_i = round(tune_i·2^64); S_i = (F_{i+1} − F_i) // (sample_{i+1} − sample_i) (floor); a knot at sample 0 with
F_0 − S_0·sample_0 where there is none; the last knot takes the slope in front of it; φ(n) = Φ_i + F_i·m + S_i·m(m − 1)/2 modulo 2^64,
m = n − sample_i, Φ continuous; (c, s) = trig16[φ >> 48]; out = (xr·c + xi·s, xi·c − xr·s) in float32, one rounding per operation.
"""
import functools
import math

import numpy as np
import tune_common as tc
from batch_common import capture

N = tc.N
M64 = (1 << 64) - 1
WINDOW = 1.0 / (2048 * 1.2)        # the tiles' tuning window at 1.2 samples per symbol: 4.07e-4 cycles per sample
F32 = np.float32
ZERO = {"cu8": 128, "cs8": 0, "cu16": 32768, "cs16": 0, "cf32": 0}


# ---- captures whose carrier moves -------------------------------------------------------------------------------------------------------
def drift_freq(n, A, T, phase):
    """f[k] = A·sin(2πk/T + phase) for k = 0 … n − 1, cycles per sample."""
    return A * np.sin(2.0 * np.pi * np.arange(n) / T + phase)


def _rotated(iq, f):
    """The cu8 capture multiplied by exp(+j2π·Σ_{k<n} f[k]) and requantised to u8 (batch_common.shifted's rounding)."""
    a = iq.reshape(-1, 2).astype(np.float64) - 128
    ph = np.concatenate([[0.0], np.cumsum(f)[:-1]])
    z = (a[:, 0] + 1j * a[:, 1]) * np.exp(2j * np.pi * ph)
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1) + 128), 0, 255).astype(np.uint8).reshape(-1)


def drifted(iq, A, T, phase):
    """The capture with a carrier offset of A·sin(2πn/T + phase)."""
    return _rotated(iq, drift_freq(len(iq) // 2, A, T, phase))


def ramp_freq(n, f0, f1):
    return np.linspace(f0, f1, n)


def ramped(iq, f0, f1):
    """The capture with a carrier offset that runs linearly from f0 to f1 over its length."""
    return _rotated(iq, ramp_freq(len(iq) // 2, f0, f1))


@functools.lru_cache(maxsize=None)
def drifted_capture(noise, A, phase, n_packets=1000):
    """drifted(capture(n_packets, 11, noise)) with T = the capture's length: (cu8 items, f[n])."""
    iq = capture(n_packets, 11, noise)[0]
    n = len(iq) // 2
    return drifted(iq, A, n, phase), drift_freq(n, A, n, phase)


# ---- the tracker ----------------------------------------------------------------------------------------------------------------------------
def frame_starts(n, blocks=4, hop=65536):
    if n < blocks * N:
        return []
    starts = list(range(0, n - blocks * N + 1, hop))
    e = (n - blocks * N) // N * N
    return starts + ([e] if e > starts[-1] else [])


def spectrum(z, blocks):
    """P of tune_common.estimate for the first `blocks` blocks of z."""
    P = np.zeros(N)
    for b in range(blocks):
        zb = z[b * N:(b + 1) * N]
        rms = np.sqrt(np.mean(np.abs(zb) ** 2))
        zb = zb / rms if rms > 0 else np.zeros(N, np.complex128)
        z2 = zb * zb
        P += np.abs(np.fft.fft(z2 * z2)) ** 2
    return P


def track(z, blocks=4, hop=65536, span=64, min_quality=30.0):
    """The tracker on the complex samples z: dict(frames: [dict(center, tune, quality, bin, held, power, mean_power)], accepted, tune_first,
    tune_last, tune_min, tune_max, quality_min)."""
    z = np.asarray(z, np.complex128)
    frames, b = [], None
    for s in frame_starts(len(z), blocks, hop):
        zf = z[s:s + blocks * N]
        if b is None or span == 0:
            e = tc.estimate(zf, blocks)
            rec = dict(tune=e["tune"], quality=e["quality"], bin=e["bin"], power=e["power"], mean_power=e["mean_power"])
        else:
            P = spectrum(zf, blocks)
            bins = (b - span + np.arange(2 * span + 1)) % N
            k0 = int(bins[int(np.argmax(P[bins]))])
            l, c, r, mean = float(P[(k0 - 1) % N]), float(P[k0]), float(P[(k0 + 1) % N]), float(P.mean())
            rec = dict(tune=tc.tune_from_peak(k0, l, c, r), quality=c / mean if c > 0 else 0.0, bin=k0, power=[l, c, r], mean_power=mean)
        rec["center"], rec["held"] = s + blocks * N // 2, 0 if rec["quality"] >= min_quality else 1
        if not rec["held"]:
            b = rec["bin"]
        frames.append(rec)
    acc = [f for f in frames if not f["held"]]
    t = [f["tune"] for f in acc] or [0.0]
    return dict(frames=frames, accepted=len(acc), tune_first=t[0], tune_last=t[-1], tune_min=min(t), tune_max=max(t),
                quality_min=min([f["quality"] for f in acc] or [0.0]))


def knots_of(frames):
    return [(f["center"], f["tune"]) for f in frames if not f["held"]]


def track_value(knots, n):
    """The piecewise-linear track through the knots at the samples 0 … n − 1, the first and the last slope run on outside them (float64)."""
    x = np.arange(n, dtype=np.float64)
    if not knots:
        return np.zeros(n)
    ks, kt = np.array([k[0] for k in knots], np.float64), np.array([k[1] for k in knots], np.float64)
    if len(knots) == 1:
        return np.full(n, kt[0])
    y = np.interp(x, ks, kt)
    lo, hi = x < ks[0], x > ks[-1]
    y[lo] = kt[0] + (x[lo] - ks[0]) * (kt[1] - kt[0]) / (ks[1] - ks[0])
    y[hi] = kt[-1] + (x[hi] - ks[-1]) * (kt[-1] - kt[-2]) / (ks[-1] - ks[-2])
    return y


# ---- the derotator ------------------------------------------------------------------------------------------------------------------------
def freq_word(tune):
    """round(tune·2^64) as a Python integer (exact: a double times a power of two)."""
    num, den = float(tune).as_integer_ratio()
    q, r = divmod(num << 64, den)
    if 2 * r > den or (2 * r == den and q & 1):                     # to nearest, ties to even (llrint's default mode)
        q += 1
    return q


def knot_error(knots):
    """0, or (rule, knot) where the knots break a rule of lsdr_derotate_batch: 1 a sample ≥ 2^31, 2 samples not strictly ascending, 3 a tune
    not finite or outside (−0.5, 0.5), 4 a step of 0.5 or more between neighbours."""
    for i, (s, t) in enumerate(knots):
        if s >= 1 << 31:
            return 1, i
        if i and s <= knots[i - 1][0]:
            return 2, i
        if not math.isfinite(t) or not abs(t) < 0.5:
            return 3, i
        if i and (not abs(t - knots[i - 1][1]) < 0.5 or abs(freq_word(t) - freq_word(knots[i - 1][1])) >= 1 << 63):
            return 4, i
    return 0


def segments(knots):
    """[(start, Φ, F, S)] in Python integers, Φ, F and S modulo 2^64."""
    if not knots:
        return [(0, 0, 0, 0)]
    F = [freq_word(t) for _, t in knots]
    s = [int(k[0]) for k in knots]
    slope = lambda i: 0 if len(knots) == 1 else (F[min(i, len(knots) - 2) + 1] - F[min(i, len(knots) - 2)]) // (s[min(i, len(knots) - 2) + 1] - s[min(i, len(knots) - 2)])
    segs = []
    if s[0] > 0:
        segs.append((0, 0, (F[0] - slope(0) * s[0]) & M64, slope(0) & M64))
    for i in range(len(knots)):
        phi = phase(segs[-1], s[i]) if segs else 0
        segs.append((s[i], phi, F[i] & M64, slope(i) & M64))
    return segs


def phase(seg, n):
    start, phi, F, S = seg
    m = n - start
    return (phi + F * m + S * (m * (m - 1) // 2)) & M64


def segment_of(segs, n):
    return max(i for i, g in enumerate(segs) if g[0] <= n)


def phases(knots, n):
    """φ(0 … n − 1) as numpy uint64 (wrapping arithmetic, segment by segment)."""
    segs = segments(knots)
    out = np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        for i, (start, phi, F, S) in enumerate(segs):
            end = min(n, segs[i + 1][0] if i + 1 < len(segs) else n)
            if end <= start:
                continue
            m = np.arange(end - start, dtype=np.uint64)
            tri = np.where(m > 0, m * (m - np.uint64(1)) // np.uint64(2), np.uint64(0)).astype(np.uint64)       # m < 2^32: m(m − 1) < 2^64
            out[start:end] = np.uint64(phi) + np.uint64(F) * m + np.uint64(S) * tri
    return out


def convert(items, fmt="cu8", scale=1.0):
    """(xr, xi) float32 of the items (interleaved I, Q): float(item − Z)·scale, one rounding per component, like the device's loads."""
    a = np.asarray(items).reshape(-1, 2)
    sc = F32(scale if scale else 1.0)
    if fmt == "cf32":
        return a[:, 0].astype(F32) * sc, a[:, 1].astype(F32) * sc
    v = (a.astype(np.int64) - ZERO[fmt]).astype(F32)
    return v[:, 0] * sc, v[:, 1] * sc


def derotate(items, knots, trig, fmt="cu8", scale=1.0):
    """The derotator's output (complex64) for the items and the knots; trig: capi.trig16()."""
    xr, xi = convert(items, fmt, scale)
    idx = (phases(knots, len(xr)) >> np.uint64(48)).astype(np.int64)
    c, s = trig.real[idx].astype(F32), trig.imag[idx].astype(F32)
    out = np.empty(len(xr), np.complex64)
    out.real = xr * c + xi * s
    out.imag = xi * c - xr * s
    return out
