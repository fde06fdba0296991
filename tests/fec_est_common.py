"""lsdr_fec_est's definition (include/lsdr_hip.h) restated in numpy — a test oracle, never imported by the product — and the captures
the code-rate tests share.

counts(sym) evaluates readerrors() (dvb.h:391-412) of a freshly constructed deconvol_sync for every (rate, alignment, skip), vectorised
over the refills, with the polynomials of oracle.deconv_info(rate); estimate(sym) applies the exact-fraction rules and returns the record
as the dict capi.FecEstimator returns it.
"""
import functools

import numpy as np

RATES = (0, 1, 3, 4, 5)                                   # LSDR_FEC12, 23 (scored as 4/6), 34, 56, 78: the record's order
NAMES = {0: "1/2", 1: "2/3", 3: "3/4", 4: "5/6", 5: "7/8"}
NOISE = 7.5


def luts():
    """init_syncs (dvb.h:308-360): lut[alignment][symbol & 3] = I << 1 | Q; symbol bit 1 is re_pos, bit 0 im_pos (dvb.h:373)."""
    out = np.zeros((4, 4), np.uint64)
    for sym in range(4):
        re_pos, im_pos = (sym >> 1) & 1, sym & 1
        re_neg = 1 - re_pos
        iq = [(0 if re_pos else 1, 0 if im_pos else 1), (0 if im_pos else 1, 0 if re_neg else 1),
              (0 if re_pos else 1, 1 if im_pos else 0), (1 if im_pos else 0, 0 if re_neg else 1)]
        for a, (i, q) in enumerate(iq):
            out[a, sym] = (i << 1) | q
    return out


LUTS = luts()


@functools.lru_cache(maxsize=None)
def _oracle():
    import pyoracle
    return pyoracle.Oracle()


@functools.lru_cache(maxsize=None)
def polys(rate):
    """(deconv, deconv2, punctperiod, punctweight) of the oracle's deconvol_sync."""
    d, d2, pp, pw = _oracle().deconv_info(rate)
    return tuple(int(v) for v in d), tuple(int(v) for v in d2), int(pp), int(pw)


def parity64(x):
    x = x.copy()
    for s in (32, 16, 8, 4, 2, 1):
        x ^= x >> np.uint64(s)
    return (x & np.uint64(1)).astype(np.int64)


def windows(bits):
    """W[p]: the 32 mapped symbols p … p + 31 as iq_t holds them behind a refill that shifted p + 31 in last (newest in the low bits)."""
    m = len(bits) - 31
    w = np.zeros(max(m, 0), np.uint64)
    for i in range(32):
        w |= bits[i:i + m] << np.uint64(62 - 2 * i)
    return w


def counts(sym):
    """{(rate, alignment, skip): (E, C)} over the hard symbols sym (any integer array; `& 3` is applied)."""
    s = np.asarray(sym).astype(np.int64) & 3
    n = len(s)
    out = {}
    for a in range(4):
        w = windows(LUTS[a][s]) if n >= 32 else np.zeros(0, np.uint64)
        for r in RATES:
            d, d2, pp, pw = polys(r)
            half = pw // 2
            for k in range(half):
                refills = (n - k - 32) // half + 1 if n - k >= 32 else 0
                wq = w[k:k + (refills - 1) * half + 1:half] if refills else w[:0]
                assert len(wq) == refills
                e = 0
                for b in range(pp):
                    e += int(np.sum(parity64(wq & np.uint64(d[b])) != parity64(wq & np.uint64(d2[b]))))
                out[(r, a, k)] = (e, refills * pp)
    return out


def less(e1, c1, e2, c2):
    if c1 == 0:
        return False
    if c2 == 0:
        return True
    return e1 * c2 < e2 * c1


def frac(e, c):
    return float(np.float32(np.float64(e) / np.float64(c))) if c else 0.0


def estimate(sym, max_symbols=None):
    """The record of one stream: the dict of capi.FecEstimate.as_dict()."""
    s = np.asarray(sym)
    if max_symbols is not None:
        s = s[:max_symbols]
    n = len(s)
    cnt = counts(s)
    score = []
    for r in RATES:
        half = polys(r)[3] // 2
        best = dict(errors=0, checks=0, sync=0, skip=0)
        for a in range(4):
            for k in range(half):
                e, c = cnt[(r, a, k)]
                if less(e, c, best["errors"], best["checks"]):
                    best = dict(errors=e, checks=c, sync=a, skip=k)
        score.append(best)
    zero = dict(errors=0, checks=0, sync=0, skip=0)
    rec = dict(fec=-1, locked=0, ambiguous=0, sync=0, skip=0, symbols=0, error_rate=0.0, runner_up=0.0, score=[dict(zero) for _ in RATES])
    win = 0
    for i in range(1, 5):
        if less(score[i]["errors"], score[i]["checks"], score[win]["errors"], score[win]["checks"]):
            win = i
    if score[win]["checks"] == 0:
        return rec
    lock = [sc["checks"] > 0 and 3 * sc["errors"] <= sc["checks"] for sc in score]
    other = None
    for i in range(5):
        if i != win and (other is None or less(score[i]["errors"], score[i]["checks"], score[other]["errors"], score[other]["checks"])):
            other = i
    w = score[win]
    rec.update(fec=RATES[win], locked=int(lock[win]), ambiguous=int(lock[win] and sum(lock) > 1), sync=w["sync"], skip=w["skip"], symbols=n,
               error_rate=frac(w["errors"], w["checks"]), runner_up=frac(score[other]["errors"], score[other]["checks"]), score=score)
    return rec


def fractions(rec):
    """[E/C per rate] of a record, float64 (nan where nothing was scored)."""
    return [sc["errors"] / sc["checks"] if sc["checks"] else float("nan") for sc in rec["score"]]


@functools.lru_cache(maxsize=None)
def capture(rate):
    """The cu8 capture of the tests at code rate `rate`, 1.2 samples per symbol, noise 7.5 per component: (IQ items, transmitted packets)."""
    from leansdr_amd import synth_dvbs
    ts = synth_dvbs.ts_packets(16)
    y = _oracle().tx_chain(ts, 6, 5, amp=75.0, cstln=1, rate=rate).astype(np.complex128)
    rng = np.random.default_rng(7 + rate)
    y = y + (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y))) * NOISE
    iq = np.empty(2 * len(y), np.uint8)
    iq[0::2] = np.clip(np.rint(y.real + 128), 0, 255)
    iq[1::2] = np.clip(np.rint(y.imag + 128), 0, 255)
    return iq, {bytes(p) for p in ts}


def conjugate_u8(iq):
    a = iq.reshape(-1, 2).copy()
    a[:, 1] = 255 - a[:, 1]
    return np.ascontiguousarray(a).reshape(-1)


def oracle_decisions(iq):
    """`symbol & 3` of the oracle's serial cstln_receiver (linear sampler, omega 1.2) on a cu8 capture, from its first symbol."""
    import pyoracle as po
    a = iq.reshape(-1, 2).astype(np.float32) - np.float32(128)
    x = (a[:, 0] + 1j * a[:, 1]).astype(np.complex64)
    out = _oracle().rx(po.rx_params(sampler=1, cstln=1, omega=1.2), x)
    return (out["sym"]["symbol"] & 3).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def decisions(rate, variant="as generated"):
    iq = capture(rate)[0]
    if variant == "conjugate":
        iq = conjugate_u8(iq)
    elif variant != "as generated":
        import batch_common
        iq = batch_common.rotate_u8(iq, int(variant))
    return oracle_decisions(iq)
