"""Shared inputs of the per-constellation / per-code-rate tests of the exact paths (test_oracle_vs_ref.py, test_oracle_golden.py,
test_gpu_rx_modcods.py, test_gpu_tx_blocks.py): one constellation with one code rate each, five receiver settings, and the block
parameters of the transmit chain.  Everything here is deterministic, so the CPU tests pin exactly what the GPU tests use."""
import hashlib
import numpy as np
import pyoracle as po

# (constellation, code rate): BPSK 1/2, QPSK 7/8, 8PSK 2/3, 16APSK 3/4, 32APSK 4/5, 64APSK 5/6, 16QAM 3/4, 64QAM 5/6, 256QAM 7/8
MODCODS = [(0, 0), (1, 5), (2, 1), (3, 3), (4, 6), (5, 4), (6, 3), (7, 4), (8, 5)]
NSYMBOLS = {0: 2, 1: 4, 2: 8, 3: 16, 4: 32, 5: 64, 6: 16, 7: 64, 8: 256}
CAPTURE_LEN = 32768

# variant: (interp, decim, sigma, loud, freq, allow_drift, pll_adjustment, meas_decimation)
#   sps3_loud_drift: |I|, |Q| above 127, the range-folding loop of the table lookup on dense tables
#   clamp: the only setting at which the !allow_drift reset fires, which makes the per-constellation divisor of the frequency limits visible
VARIANTS = {
    "sps4": (4, 1, 2.0, 1.0, 0.0, 0, 1 / 6.0, 1024),
    "sps1p2": (6, 5, 2.0, 1.0, 0.0, 0, 1 / 6.0, 1024),
    "sps3_loud_drift": (3, 1, 2.0, 7.0, 0.002, 1, 1 / 6.0, 1024),
    "sps8_offset": (8, 1, 2.0, 1.0, -0.01, 0, 1 / 6.0, 1024),
    "clamp": (4, 1, 8.0, 1.0, 0.0, 0, 100.0, 256),
}

# receiver cases of the CPU sweep: every MODCOD x every variant x nearest / linear, plus the FIR sampler twice
RX_SWEEP = [(c, r, v, s) for (c, r) in MODCODS for v in VARIANTS for s in (0, 1)] + [(3, 3, "sps4", 2), (7, 4, "sps4", 2)]
# what the GPU's serial receiver is held to: linear everywhere, nearest at three variants, FIR twice
RX_GPU = [(c, r, v, 1) for (c, r) in MODCODS for v in VARIANTS] + \
         [(c, r, v, 0) for (c, r) in MODCODS for v in ("sps4", "sps1p2", "clamp")] + [(3, 3, "sps4", 2), (7, 4, "sps4", 2)]

# transmit blocks
TX_PAIRS = [(0, 0), (1, 0), (2, 1), (3, 1), (3, 3), (3, 8), (4, 3), (4, 6), (4, 8), (5, 0), (5, 4), (6, 3), (7, 4), (8, 5)]
FEC_BITS = {0: (1, 2), 1: (2, 3), 2: (4, 6), 3: (3, 4), 4: (5, 6), 5: (7, 8), 6: (4, 5)}    # rate: (bits_in, bits_out), dvb.h:553-565
# every rate with every bits-per-symbol value that divides its bits_out (dvb.h:585)
CONVOL_PAIRS = [(rate, bps) for rate, (_, bo) in sorted(FEC_BITS.items()) for bps in range(1, 9) if bo % bps == 0]
CONVOL_NBYTES = 2520                                       # a whole number of groups at every rate (bits_in 1, 2, 3, 4, 5, 7)
RESAMPLER_CASES = [(41, 4, 0.0), (61, 6, 0.01), (5, 8, 0.0), (31, 3, -0.2), (101, 7, 0.05)]
RESAMPLER_DIVIDING = [(21, 1, 0.0), (40, 4, 0.0), (8, 8, 0.05)]   # interp divides ncoeffs: the bounded count holds one sample back
RESAMPLER_N_IN = 3000


def case_id(case):
    c, r, v, s = case
    return f"c{c}r{r}-{v}-s{s}"


_cache = {}


def capture(oracle, cstln, rate, variant, seed=None):
    """One signal: transmit chain -> + noise -> x loud -> rotated by freq cycles per sample -> complex64, at most CAPTURE_LEN samples.
    Cached and read-only: the tests share it."""
    key = (cstln, rate, variant, seed)
    if key not in _cache:
        from leansdr_amd import synth_dvbs
        interp, decim, sigma, loud, freq = VARIANTS[variant][:5]
        y = oracle.tx_chain(synth_dvbs.ts_packets(64), interp, decim, amp=75.0, cstln=cstln, rate=rate).astype(np.complex128)
        rng = np.random.default_rng(cstln * 16 + rate if seed is None else seed)
        y = y + sigma * (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y)))
        y = y * loud * np.exp(2j * np.pi * freq * np.arange(len(y)))
        x = y.astype(np.complex64)[:CAPTURE_LEN].copy()
        x.flags.writeable = False
        _cache[key] = x
    return _cache[key]


FIR_LEVEL = np.float32(16)     # rrc_rx sums to 1 over all taps: each of its 16 phases, which is what one symbol sees, to about 1/16


def rx_input(oracle, cstln, rate, variant, sampler):
    """The capture a receiver case runs on.  The FIR-sampler cases get it 16 times louder (as test_cstln_receiver_fir_sampler feeds
    these taps): at the plain level they decide only 4 distinct symbols, at this one all 16 of 16APSK and all 64 of 64QAM, so the
    coverage condition of test_oracle_vs_ref.py holds for them as for every other case."""
    key = (cstln, rate, variant, "in", sampler == 2)
    if key not in _cache:
        x = capture(oracle, cstln, rate, variant)
        if sampler == 2:
            x = x * FIR_LEVEL
            x.flags.writeable = False
        _cache[key] = x
    return _cache[key]


def rx_kwargs(cstln, rate, variant, sampler, rrc=None):
    """Keyword arguments shared by pyoracle.rx_params and capi.CstlnReceiver / capi.RxBatch."""
    interp, decim, _, _, freq, drift, pll, meas = VARIANTS[variant]
    kw = dict(sampler=sampler, cstln=cstln, fec=rate, omega=float(np.float32(interp / decim)), freq=freq, pll_adjustment=pll,
              allow_drift=drift, meas_decimation=meas)
    if sampler == 2:
        kw.update(coeffs=rrc, subsampling=16)
    return kw


_rx_cache = {}


def oracle_rx(oracle, case, rrc=None):
    """The oracle's one-shot result of a receiver case, computed once and shared."""
    if case not in _rx_cache:
        c, r, v, s = case
        _rx_cache[case] = oracle.rx(po.rx_params(**rx_kwargs(c, r, v, s, rrc)), rx_input(oracle, c, r, v, s))
    return _rx_cache[case]


def state_vec(st):
    """The receiver's loop state as (float32 vector, meas_count)."""
    d = st.as_dict()
    keys = ["mu", "phase", "freqw", "agc_gain", "est_insp", "est_sp", "est_ep", "freq_tap", "min_freqw", "max_freqw"]
    return np.array([d[k] for k in keys] + d["hist"], np.float32), int(d["meas_count"])


def state_bytes(st):
    v, count = state_vec(st)
    return v.tobytes() + np.uint64(count).tobytes()


def sha(a):
    return hashlib.sha256(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()).digest()


def rx_digest(r, x):
    """What tests/golden/modcod.npz stores per receiver case: lengths and SHA-256 of the input, of each output and of the state."""
    return dict(n=np.array([len(x), len(r["sym"]), len(r["freq"]), len(r["cstln"])], np.int64),
                sha=np.frombuffer(b"".join([sha(x), sha(r["sym"]["cost"]), sha(r["sym"]["symbol"]), sha(r["freq"]), sha(r["ss"]),
                                            sha(r["mer"]), sha(r["cstln"]), sha(state_bytes(r["state"]))]), np.uint8).reshape(8, 32))


DIGEST_FIELDS = ("input", "cost", "symbol", "freq", "ss", "mer", "cstln", "state")


def convol_input():
    return np.random.default_rng(585).integers(0, 256, CONVOL_NBYTES, dtype=np.uint8)


def tx_symbols(cstln):
    """Every symbol value of the constellation once, then 1000 random ones."""
    n = NSYMBOLS[cstln]
    return np.concatenate([np.arange(n), np.random.default_rng(1196 + cstln).integers(0, n, 1000)]).astype(np.uint8)


def resampler_input(n=RESAMPLER_N_IN):
    rng = np.random.default_rng(306)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 40).astype(np.complex64)


def resampler_coeffs(ncoeffs):
    """Taps with no symmetry and no zeros, so that a tap read out of order or dropped shows."""
    return (np.random.default_rng(290 + ncoeffs).standard_normal(ncoeffs) / np.sqrt(ncoeffs)).astype(np.float32)
