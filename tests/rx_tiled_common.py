"""Shared by tests/test_oracle_rx_tile_emulation.py (CPU) and tests/test_gpu_rx_tiled_constellations.py (GPU): the streams, the
cases and a restatement of the tiled receiver's algorithm with the oracle's serial receiver alone.

The tiled mode (LSDR_RX_TILED, cstln_receiver.hip) cuts a run into tiles.  Tile 0 continues from the carried loop state and is
one warm-up long; every other tile starts `W` samples early from the carried state with mu = phase = 0 and an empty history,
re-acquires timing and carrier phase over that warm-up and keeps the symbols of its body of `L` samples.  A tile's carrier loop
locks on the nearest of the constellation's R rotations, so its symbols are relabelled by the rotation that puts them back into
the frame of tile 0.  emulate_tiles() does just that with oracle.rx(): it says what the ALGORITHM gives with the reference's own
arithmetic, which is where the bounds of leansdr_amd/tolerance.py for BPSK and 8PSK come from, and which conditions (every
rotation taken, no tile unlocked) a stream has to meet before a GPU test on it means anything.
"""
import ctypes as C

import numpy as np
import pyoracle as po
from leansdr_amd import synth_dvbs

CHUNK = 128
ACQ = 40960                      # samples the serial receiver acquires on before the tiles take over
SPS = 4

# (name, constellation, code rate, Es/N0 in dB, TS packets, tolerance dict's name in leansdr_amd.tolerance)
# Packets: the fewest that leave more than 300 tiles of 256 samples behind ACQ, so that the seam scan crosses a kSeamBlock of 256
# tiles (a packet is 204·8 / (bits per symbol · code rate) symbols of 4 samples: 13056 / 6528 / 3264 samples).
CASES = [
    dict(name="bpsk12", cstln=0, fec=0, snr_db=12.0, packets=21, tol="TOL_BPSK"),
    dict(name="qpsk12_table", cstln=1, fec=0, snr_db=20.0, packets=30, tol="TOL"),
    dict(name="psk8_23", cstln=2, fec=1, snr_db=26.0, packets=48, tol="TOL_PSK8"),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
# (tile_len, tile_warmup) in samples: the geometries at which the reference-only conditions hold for every case
# (tests/test_oracle_rx_tile_emulation.py asserts them)
GEOMETRIES = [(1024, 1024), (512, 512), (256, 1024)]
# the drift case of the GPU test: the QPSK stream shifted by a further DRIFT_FREQ cycles per sample, receiver tuned there
DRIFT_FREQ = 1e-3


def rx_kwargs(case, **more):
    """Receiver parameters of a case, as keywords of both po.rx_params and capi.CstlnReceiver."""
    kw = dict(sampler=1, cstln=case["cstln"], fec=case["fec"], omega=float(SPS), meas_decimation=4096,
              pll_adjustment=1.0 if case["cstln"] == 1 else 1.0 / 6.0)
    kw.update(more)
    return kw


def make_stream(oracle, cstln, fec, packets, snr_db, cfo=3e-5, phase0=0.1, seed=1):
    """leandvbtx's chain at 4 samples per symbol (oracle.tx_chain on leantsgen's packets) + complex AWGN at Es/N0 = snr_db +
    a carrier at `cfo` cycles per sample starting `phase0` cycles off, so that the carrier phase — and with it the rotation
    a tile locks on — walks through every rotation of the constellation; RMS 75.  Deterministic, CPU only."""
    y = oracle.tx_chain(synth_dvbs.ts_packets(packets), interp=SPS, amp=75.0, cstln=cstln, rate=fec).astype(np.complex128)
    ps = float(np.mean(np.abs(y) ** 2))
    nstd = np.sqrt(0.5 * SPS * ps / 10 ** (snr_db / 10))          # Es/N0 in the symbol-rate bandwidth, as leansdr_amd.synth
    rng = np.random.default_rng(seed)
    y = y + (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y))) * nstd
    y = y * np.exp(2j * np.pi * (cfo * np.arange(len(y)) + phase0))
    y *= 75.0 / np.sqrt(np.mean(np.abs(y) ** 2))
    return y.astype(np.complex64)


def case_stream(oracle, case, shift=0.0):
    x = make_stream(oracle, case["cstln"], case["fec"], case["packets"], case["snr_db"])
    if shift:
        x = (x.astype(np.complex128) * np.exp(2j * np.pi * shift * np.arange(len(x)))).astype(np.complex64)
    return x


def acquire(oracle, params, x):
    """Serial acquisition over the first ACQ samples and the serial continuation over the rest: (state at ACQ, reference)."""
    a = oracle.rx(params, x[:ACQ + 1])
    assert a["consumed"] == ACQ
    return a["state"], oracle.rx(params, x[ACQ:], state_in=a["state"])


def copy_state(st, **fields):
    c = po.RxState.from_buffer_copy(bytes(st))
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def tile_spans(n_samples, L, W, readahead=1):
    """[(first sample, end sample)] of every tile's body for a run over n_samples: tile 0 is one warm-up long, the others L,
    the last one what is left (rx_tiled_plan in cstln_receiver.hip)."""
    chunks = (n_samples - readahead) // CHUNK if n_samples >= CHUNK + readahead else 0
    end = chunks * CHUNK
    spans = [(0, min(W, end))]
    s = W
    while s < end:
        spans.append((s, min(s + L, end)))
        s += L
    return spans


def relabel_table(oracle, cstln, fec):
    """relabel[k][s]: the symbol whose point is nearest to point s turned by +k·360°/R (lsdr_rx_create builds the same)."""
    lut = oracle.cstln_lut(cstln, fec)
    R, pts = lut["nrotations"], lut["symbols"].astype(np.float64)
    z = pts[:, 0] + 1j * pts[:, 1]
    tab = np.zeros((R, len(z)), np.uint8)
    for k in range(R):
        zr = z * np.exp(2j * np.pi * k / R)
        tab[k] = np.argmin(np.abs(zr[:, None] - z[None, :]), axis=1)
    return tab


class SerialRx:
    """oracle.rx() on ONE lo_rx handle (its constellation table is built once, not per call): run(x, state) continues the serial
    receiver from `state` over x and returns (symbols, state after); the whole of x but its read-ahead sample must be consumed."""

    def __init__(self, oracle, params):
        self.lib, self.params = oracle.lib, params
        self.h = self.lib.lo_rx_new(C.byref(params))

    def close(self):
        if self.h:
            self.lib.lo_rx_free(self.h)
            self.h = None

    def run(self, x, state):
        x = np.ascontiguousarray(x, np.complex64)
        self.lib.lo_rx_set_state(self.h, C.byref(state))
        out = np.zeros(len(x) + 256, po.SOFTSYM)
        consumed = C.c_size_t()
        n = self.lib.lo_rx_run(self.h, x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p), len(out), C.byref(consumed),
                               None, None, None, 0, None, None, 0, None)
        assert consumed.value == len(x) - 1, (consumed.value, len(x))
        st = po.RxState()
        self.lib.lo_rx_get_state(self.h, C.byref(st))
        return out[:n], st


def serial_by_span(oracle, params, x, state, spans):
    """The serial receiver run span by span (bit for bit one run: its whole state is carried): per span the index of its first
    symbol in the serial output and the loop's mu at the span's first sample; and all symbols."""
    rx = SerialRx(oracle, params)
    st, first, mus, syms, n = state, [], [], [], 0
    for s, e in spans:
        first.append(n); mus.append(st.mu)
        sym, st = rx.run(x[s:e + 1], st)
        syms.append(sym); n += len(sym)
    rx.close()
    return np.array(first), np.array(mus), np.concatenate(syms)


def emulate_tiles(oracle, params, x_after_acq, state, L, W, serial=None):
    """The tiled algorithm with the oracle alone.  Tile 0 continues over x[0 : W] from `state`; a tile whose body starts at
    sample s runs oracle.rx over x[s−W : s+1] from `state` with mu = phase = 0 and the history cleared, goes on over its body,
    and its body's decisions are relabelled by the best of the R rotations against the serial receiver's.

    Alignment is by symbol counts: the serial receiver, run span by span, says which of its symbols is the first at or behind
    sample s and how far (mu) that symbol's instant lies behind s; the tile's own mu at s is the same instant, or a whole number
    of symbols away from it (the tile put a symbol just before s that the serial loop puts just behind it, or the other way
    round): round((mu_tile − mu_serial) / omega) symbols.  A serial symbol that two tiles produce keeps the first one's; one that
    no tile produces counts as a wrong decision.

    Returns dict(sym: the serial output's layout filled with the tiles' relabelled symbols, filled: mask, ref: serial symbols,
    rot: per-tile rotation, share: per-tile share of decisions equal to serial, equal: overall share, dcost: |Δcost| of the
    filled symbols, spans)."""
    x = x_after_acq
    spans = tile_spans(len(x), L, W)
    first, mus, ref = serial if serial is not None else serial_by_span(oracle, params, x, state, spans)
    relabel = relabel_table(oracle, params.cstln, params.fec)
    R = len(relabel)
    out = np.zeros(len(ref), po.SOFTSYM)
    filled = np.zeros(len(ref), bool)
    rot, share = [], []
    start = copy_state(state, mu=0.0, phase=0.0)
    for i in range(12):
        start.hist[i] = 0.0
    rx = SerialRx(oracle, params)
    for j, (s, e) in enumerate(spans):
        if j == 0:
            (body, _), warm, k = rx.run(x[s:e + 1], state), None, 0
        else:
            warm, wst = rx.run(x[s - W:s + 1], start)
            body, _ = rx.run(x[s:e + 1], wst)
            k = int(np.rint((wst.mu - mus[j]) / params.omega))
        # (the last warm-up symbol rides along: where the tile put a symbol just before s that the serial loop puts behind it and
        # the tile before did not reach, the seam takes it from the warm-up — the kernel's seam repair does the same)
        pre = warm[-1:] if j else body[:0]
        t = np.concatenate([pre, body])
        idx = first[j] + k - len(pre) + np.arange(len(t))
        ok = (idx >= 0) & (idx < len(ref))
        t, idx = t[ok], idx[ok]
        own = np.arange(len(t)) >= len(pre)                                # the body's symbols: what the tile is judged by
        own = own[ok]
        hits = [(relabel[r][t["symbol"][own]] == ref["symbol"][idx[own]]).sum() for r in range(R)]
        r = int(np.argmax(hits)) if j else 0
        rot.append(r); share.append(hits[r] / max(1, int(own.sum())))
        t = t.copy(); t["symbol"] = relabel[r][t["symbol"]]
        new = ~filled[idx]
        out[idx[new]] = t[new]; filled[idx[new]] = True
    rx.close()
    same = (out["symbol"] == ref["symbol"]) & filled
    dcost = np.abs(out["cost"].astype(np.int64) - ref["cost"].astype(np.int64))[filled]
    return dict(sym=out, filled=filled, ref=ref, rot=np.array(rot), share=np.array(share), equal=float(same.mean()),
                dcost=dcost, spans=spans)


def figures(em):
    """The figures the bounds of leansdr_amd.tolerance are taken from."""
    d = em["dcost"]
    return dict(tiles=len(em["spans"]), equal=em["equal"], min_tile=float(em["share"][1:].min()) if len(em["share"]) > 1 else 1.0,
                rotations=sorted(set(int(r) for r in em["rot"][1:])), mean_dcost=float(d.mean()), p99_dcost=float(np.percentile(d, 99)),
                max_dcost=int(d.max()), missing=int((~em["filled"]).sum()), max_abs_cost=int(np.abs(em["ref"]["cost"].astype(np.int64)).max()))
