"""Shared helpers of the carrier scan's tests (lsdr_carrier_scan, include/lsdr_hip.h): the scan restated in numpy — a test oracle, never
imported by the product — and the wideband captures the CPU and the GPU tests share.

The scan (the header states it the same way).  For one capture of n items, N = 4096:
  1 M = min(blocks, n // N) whole blocks; block b starts at sample b·stride·N, stride = 1, or with spread max(1, (n // N) // blocks);
  2 per block z·w with the Hann window w[n] = 0.5 − 0.5·cos(2πn/N), X = FFT_N, |X[k]|² of all bins;
  3 P[k] = Σ_blocks |X[k]|² in block order;
  4 S[k] = (Σ_{j=−smooth…+smooth} P[(k+j) mod N]) / (2·smooth + 1), j ascending;
  5 floor = the value of rank N/8 (from 0) of S; T = floor·factor, factor = float32(10^(threshold_db/10));
  6 above[k] = S[k] ≥ T; a run starts at s where above[s] and not above[s−1] (cyclic) and lasts while above holds; runs in ascending
    (s + N/2) mod N; all above: saturated, no carriers; runs shorter than min_bins are dropped, `found` counts the rest, the first
    max_carriers are listed;
  7 per listed run [a, b] (unwrapped, S indexed mod N), n = b − a + 1, q = n // 4, in double: plateau = Σ_{k=a+q…b−q} S[k] / (n − 2q),
    sequential; L = plateau − floor; H = floor + L/2; H < T: weak, lo = a − 0.5, hi = b + 0.5; else i = first k ≥ a with S[k] ≥ H,
    lo = i − (S[i]−H)/(S[i]−S[i−1]), j = last k ≤ b with S[k] ≥ H, hi = j + (S[j]−H)/(S[j]−S[j+1]); c = (lo+hi)/(2N),
    center = c − floor(c + 0.5); bandwidth = (hi − lo)/N; omega = 1/bandwidth; level = L/floor;
  8 M = 0: everything zero.
find(P, …, exact=False) does steps 4 to 8 in float64 (for the accuracy the definition has); exact=True does them as the device does —
S, floor and T in float32 one rounding per operation, step 7 in sequential double on those floats, the record's floats rounded last — and
has to give the device's records bit for bit from the device's own P.
"""
import functools
import math

import numpy as np

N = 4096
BLOCKS = 64
SMOOTH, THRESHOLD_DB, MAX_CARRIERS = 8, 3.0, 32
SKIP_SYMBOLS = 18000          # the generator's interleaver starts from zeros, and that start is no flat spectrum
CENTER_CAP, OMEGA_CAP = 2.0 / N, 0.03       # what the bounds may never be looser than: 2 bins, 3 %
# the worst errors of the float64 restatement on CASES with 64 blocks (test_carrier_scan_abi.py measures them again and has the figures):
# the bounds are twice these, under the caps — fine tuning then starts well inside TuneEstimator's range and RateEstimator's ±10 % window
CENTER_WORST, OMEGA_WORST = 3.7e-4, 0.0167
CENTER_BOUND, OMEGA_BOUND = min(2 * CENTER_WORST, CENTER_CAP), min(2 * OMEGA_WORST, OMEGA_CAP)
LEVEL_DB_BOUND = 0.5
# name -> ([(samples per symbol, centre in cycles per sample, amplitude)], noise std per component)
MIX_A = [(12, -0.22, 40.0), (8, 0.05, 45.0), (24, 0.33, 15.0)]
MIX_B = [(10, 0.49, 40.0), (4, 0.0, 20.0), (16, -0.3, 9.0)]
CASES = [("mix A noise 7.5", MIX_A, 7.5), ("mix A noise 18", MIX_A, 18.0), ("mix B noise 7.5", MIX_B, 7.5)]
NOISE_ALONE = 18.0
SEED = 7                      # of every capture's noise: the seed of the closed loop's wideband capture
SUMMARY_ZERO = dict(blocks=0, stride=0, found=0, listed=0, saturated=0, floor=0.0, threshold=0.0, carriers=[])


def to_complex(items):
    """cu8 items (interleaved I, Q) as complex128."""
    a = np.asarray(items).reshape(-1, 2).astype(np.float64) - 128.0
    return a[:, 0] + 1j * a[:, 1]


def to_u8(x):
    iq = np.empty(2 * len(x), np.uint8)
    iq[0::2] = np.clip(np.rint(x.real + 128), 0, 255)
    iq[1::2] = np.clip(np.rint(x.imag + 128), 0, 255)
    return iq


@functools.lru_cache(maxsize=None)
def _carrier(sps, n_packets, start, skip):
    """A carrier's baseband at unit power from `skip` symbols into its stream on (complex128)."""
    from leansdr_amd import synth_dvbs
    return synth_dvbs.modulate(synth_dvbs.ts_packets(n_packets, start=start), sps, 1)[skip * sps:]


def mix(spec, n, noise, seed, skip=SKIP_SYMBOLS, packets=None, starts=None):
    """cu8 items of n samples: the sum of synth_dvbs.modulate carriers (sps, f, amp) — each from `skip` symbols into its stream on, shifted
    to +f cycles per sample (batch_common.shifted's sign), with just enough packets (or packets[i], its stream zero behind its end), packet
    counters from starts[i] (0) — plus Gaussian noise of std `noise` per component."""
    t = np.arange(n)
    x = np.zeros(n, np.complex128)
    for i, (sps, f, amp) in enumerate(spec):
        n_packets = packets[i] if packets else -(-(n // sps + skip + 64) // 1632) + 1
        bb = _carrier(sps, n_packets, starts[i] if starts else 0, skip)[:n]
        assert packets or len(bb) == n, (sps, n_packets, len(bb))
        x[: len(bb)] += amp * bb * np.exp(2j * np.pi * f * t[: len(bb)])
    rng = np.random.default_rng(seed)
    x += (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * noise
    return to_u8(x)


@functools.lru_cache(maxsize=None)
def case(k, blocks=BLOCKS):
    """(name, spec, noise, cu8 items) of case k of CASES, blocks·N samples."""
    name, spec, noise = CASES[k]
    return name, spec, noise, mix(tuple(spec), blocks * N, noise, SEED)


@functools.lru_cache(maxsize=None)
def noise_alone(blocks=BLOCKS, seed=SEED):
    return mix((), blocks * N, NOISE_ALONE, seed)


def stride_of(n, blocks, spread):
    return max(1, (n // N) // blocks) if spread else 1


def spectrum(z, blocks=BLOCKS, spread=False):
    """Steps 1 to 3 in float64 on the complex samples z: (P float64[N], M, stride)."""
    z = np.asarray(z, np.complex128)
    M, stride = min(int(blocks), len(z) // N), stride_of(len(z), int(blocks), spread)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    P = np.zeros(N)
    for b in range(M):
        P += np.abs(np.fft.fft(z[b * stride * N:(b * stride + 1) * N] * w)) ** 2
    return P, M, stride


def smoothed(P, smooth, dtype):
    """Step 4 in `dtype`: one rounding per addition, j ascending, one division."""
    P = np.asarray(P, dtype)
    acc = np.zeros(N, dtype)
    for j in range(-smooth, smooth + 1):
        acc = acc + np.roll(P, -j)                   # np.roll(P, −j)[k] = P[(k + j) mod N]
    return acc / dtype(2 * smooth + 1)


def runs_of(above):
    """Step 6's runs of a boolean array over the N bins: [(first bin, bins)] in ascending (first + N/2) mod N; None where all are above."""
    if above.all():
        return None
    out = []
    for p in range(N):
        s = (p + N // 2) % N
        if above[s] and not above[(s - 1) % N]:
            n = 1
            while above[(s + n) % N]:
                n += 1
            out.append((s, n))
    return out


def record(S, a, n, floor, T, exact):
    """Step 7 for the run of n bins from a on.  S, floor, T: floats of the dtype in use; the arithmetic is Python's double."""
    b, q = a + n - 1, n // 4
    total = 0.0
    for k in range(a + q, b - q + 1):
        total += float(S[k % N])
    plateau = total / (n - 2 * q)
    floor, T = float(floor), float(T)
    L = plateau - floor
    H = floor + L / 2.0
    weak = H < T
    if weak:
        lo, hi = a - 0.5, b + 0.5
    else:
        i = next(k for k in range(a, b + 1) if float(S[k % N]) >= H)
        j = next(k for k in range(b, a - 1, -1) if float(S[k % N]) >= H)
        si, sj = float(S[i % N]), float(S[j % N])
        lo = i - (si - H) / (si - float(S[(i - 1) % N]))
        hi = j + (sj - H) / (sj - float(S[(j + 1) % N]))
    c = (lo + hi) / (2.0 * N)
    bw = (hi - lo) / N
    r = dict(center=c - math.floor(c + 0.5), bandwidth=bw, omega=1.0 / bw, level=L / floor, plateau=plateau)
    if exact:
        r = {k: float(np.float32(v)) for k, v in r.items()}
    r["cnr_db"] = 10.0 * math.log10(r["level"]) if r["level"] > 0 else float("-inf")
    return dict(r, first_bin=a, bins=n, weak=int(weak))


def find(P, M, stride, smooth=SMOOTH, threshold_db=THRESHOLD_DB, min_bins=0, max_carriers=MAX_CARRIERS, exact=False):
    """Steps 4 to 8 from P: CarrierScan.scan's dict of one capture."""
    if M == 0:
        return dict(SUMMARY_ZERO, carriers=[])
    dtype = np.float32 if exact else np.float64
    S = smoothed(P, smooth, dtype)
    floor = np.sort(S)[N // 8]
    factor = np.float32(10.0 ** (float(np.float32(threshold_db)) / 10.0))
    T = floor * dtype(factor)
    runs = runs_of(S >= T)
    saturated = runs is None
    kept = [r for r in runs or [] if r[1] >= (min_bins or 2 * smooth + 1)]
    listed = kept[:max_carriers]
    return dict(blocks=M, stride=stride, found=len(kept), listed=len(listed), saturated=int(saturated), floor=float(floor), threshold=float(T),
                carriers=[record(S, a, n, floor, T, exact) for a, n in listed])


def scan(z, blocks=BLOCKS, spread=False, **kw):
    """The whole scan in float64 on the complex samples z."""
    return find(*spectrum(z, blocks, spread), **kw)


def expected_level(sps, amp, noise):
    """A carrier's C/N as the scan reads it: its power density over the noise's, amp²·sps / (2·noise²)."""
    return amp * amp * sps / (2.0 * noise * noise)


def match(carriers, spec):
    """The scan's carriers paired with the spec's by centre (cyclic distance): [(carrier, (sps, f, amp))] in the spec's order; asserts that
    every carrier of the spec is the nearest of exactly one found."""
    assert len(carriers) == len(spec), (carriers, spec)
    dist = lambda a, b: abs((a - b + 0.5) % 1.0 - 0.5)
    out = []
    for s in spec:
        out.append((min(carriers, key=lambda c: dist(c["center"], s[1])), s))
    assert len({id(c) for c, _ in out}) == len(spec), (carriers, spec)
    return out


def errors(carriers, spec, noise):
    """(max |center − f| cyclic, max |omega/sps − 1|, max |level in dB − expected|) of a scan against its spec."""
    dc = do = dl = 0.0
    for c, (sps, f, amp) in match(carriers, spec):
        dc = max(dc, abs((c["center"] - f + 0.5) % 1.0 - 0.5))
        do = max(do, abs(c["omega"] / sps - 1.0))
        dl = max(dl, abs(c["cnr_db"] - 10.0 * math.log10(expected_level(sps, amp, noise))))
    return dc, do, dl


# ---- the wideband capture of the closed loop: two carriers from their first symbol on, so that the reference decodes them
WIDE_N = 6267071
WIDE = [(12, -0.11, 50.0), (10, 0.14, 50.0)]
WIDE_PACKETS, WIDE_STARTS, WIDE_NOISE, WIDE_SEED = (320, 384), (0, 100000), 7.5, 7


@functools.lru_cache(maxsize=None)
def wideband():
    return mix(tuple(WIDE), WIDE_N, WIDE_NOISE, WIDE_SEED, skip=0, packets=WIDE_PACKETS, starts=WIDE_STARTS)
