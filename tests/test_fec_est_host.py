"""lsdr_fec_est without a GPU: the polynomials the library scores with, the parity-check property the estimator rests on, and the numpy
restatement of the definition (fec_est_common) on the oracle receiver's decisions — what the device is then held to bit for bit in
test_gpu_fec_est.py.

Bounds.  The reference gives an alignment up above a disagreement fraction of 1/3 (dvb.h:449-453).  The transmitted rate's fraction must
be at most 0.2 and every other rate's at least 0.4: both sides clear of 1/3.  A wrong hypothesis is a sum of fair coins, 0.5 less the
minimum over its 4·(punctweight/2) hypotheses: 0.449 … 0.50 over 4096 symbols.
Measured here on the five captures (16 packets, 1.2 samples per symbol, noise 7.5, first 4096 symbols, acquisition included): the
transmitted rate 0.044 (1/2), 0.053 (2/3), 0.084 (3/4), 0.100 (5/6), 0.137 (7/8); every other rate at least 0.449; the same within 0.01
on the rotated and conjugated captures.  Uniformly random symbols: 0.462 over 4096, 0.487 over 16384.
"""
import numpy as np
import pytest
import fec_est_common as fc

VARIANTS = ("as generated", "1", "2", "3", "conjugate")
PUNCT = {0: (0x1, 0x1), 1: (0xa, 0xf), 3: (0x5, 0x6), 4: (0x15, 0x1a), 5: (0x45, 0x7a)}     # pX, pY (dvb.h:487-507)


def parity(x):
    return bin(x).count("1") & 1


def convolve(s, pp, punct):
    """deconvol_sync::convolve (dvb.h:165-179): the punctured code's I/Q bits for the message bits s, MSB first."""
    iq, state = 0, 0
    for b in range(s.bit_length() - 1, -1, -1):
        state = (state >> 1) | (((s >> b) & 1) << 6)
        for j, g in enumerate((0o171, 0o133)):
            if punct[j] & (1 << (b % pp)):
                iq = (iq << 1) | parity(state & g)
    return iq


def test_polys_are_the_oracles(capi):
    for r in fc.RATES:
        d, d2, pp, pw = capi.fec_polys(r)
        od, od2, opp, opw = fc.polys(r)
        assert (tuple(d), tuple(d2), pp, pw) == (od, od2, opp, opw), fc.NAMES[r]
        assert all(a != b for a, b in zip(d, d2)), fc.NAMES[r]
    assert [capi.fec_polys(r)[2:] for r in fc.RATES] == [(1, 2), (4, 6), (3, 4), (5, 6), (7, 8)]
    for other in (capi.FEC46, capi.FEC910, -1):                            # 4/6 is how 2/3 is scored, not a rate of its own
        with pytest.raises(capi.LsdrError):
            capi.fec_polys(other)


def test_the_difference_of_the_two_inverses_is_a_parity_check(capi):
    for r in fc.RATES:
        d, d2, pp, pw = capi.fec_polys(r)
        for b in range(pp):
            for i in range(64):
                assert parity(convolve(1 << i, pp, PUNCT[r]) & (d[b] ^ d2[b])) == 0, (fc.NAMES[r], b, i)


def test_noise_free_code_words_score_zero(oracle):
    """The definition on the encoder's own symbols: exactly 0 for the transmitted rate, near 1/2 for every other."""
    from leansdr_amd import synth_dvbs
    il = oracle.interleaver(oracle.rs_encoder(oracle.randomizer(synth_dvbs.ts_packets(24))))
    assert len(il) == 2652                                                 # (the interleaver keeps its first 11 packets)
    for r in fc.RATES:
        sym, _ = oracle.dvb_convol(il, 2 if r == 1 else r, 2)
        iq = oracle.cstln_transmitter(sym, 1, r)
        hard = ((iq.real > 0).astype(np.uint8) << 1) | (iq.imag > 0).astype(np.uint8)
        rec = fc.estimate(hard[:4096])
        fr = fc.fractions(rec)
        print(f"{fc.NAMES[r]}: noise-free fractions {['%.3f' % f for f in fr]}")
        assert rec["fec"] == r and rec["locked"] == 1 and rec["ambiguous"] == 0 and rec["error_rate"] == 0.0, rec
        assert min(f for i, f in enumerate(fr) if fc.RATES[i] != r) >= 0.4, fr


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_picks_the_transmitted_rate(variant):
    for r in fc.RATES:
        d = fc.decisions(r, variant)
        assert len(d) >= 4096
        rec = fc.estimate(d, 4096)
        fr = fc.fractions(rec)
        print(f"{fc.NAMES[r]} {variant}: {len(d)} symbols, fractions {['%.3f' % f for f in fr]}, sync {rec['sync']}, skip {rec['skip']}")
        assert rec["fec"] == r and rec["locked"] == 1 and rec["ambiguous"] == 0 and rec["symbols"] == 4096, rec
        win = fc.RATES.index(r)
        assert fr[win] <= 0.2, (fc.NAMES[r], variant, fr)
        assert min(f for i, f in enumerate(fr) if i != win) >= 0.4, (fc.NAMES[r], variant, fr)
        assert rec["error_rate"] == np.float32(fr[win]) and rec["runner_up"] == np.float32(min(f for i, f in enumerate(fr) if i != win))


def test_random_symbols_do_not_lock():
    rng = np.random.default_rng(99)
    for n in (4096, 16384):
        rec = fc.estimate(rng.integers(0, 4, n).astype(np.uint8))
        print(f"{n} uniformly random symbols: best fraction {rec['error_rate']:.3f}")
        assert rec["locked"] == 0 and rec["ambiguous"] == 0 and rec["error_rate"] >= 0.4, rec


def test_restatement_edges():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 4, 64).astype(np.uint8)
    zero = fc.estimate(s[:0])
    assert zero["fec"] == -1 and zero["symbols"] == 0 and fc.estimate(s[:31]) == zero
    one = fc.estimate(s[:32])                                              # one refill of skip 0 for every rate, none of any other skip
    assert one["fec"] >= 0 and [sc["checks"] for sc in one["score"]] == [1, 4, 3, 5, 7] and all(sc["skip"] == 0 for sc in one["score"])
    cnt = fc.counts(s[:36])
    assert cnt[(5, 0, 3)][1] == 7 and cnt[(5, 0, 0)][1] == 14 and cnt[(0, 0, 0)][1] == 5
    assert fc.counts(s[:35])[(5, 0, 3)][1] == 7 and fc.counts(s[:34])[(5, 0, 3)][1] == 0        # the skip bound: 32 + skip symbols
    assert fc.estimate(s, 40) == fc.estimate(s[:40])


def test_group_by_fec(capi):
    rec = lambda fec, locked=1, ambiguous=0: dict(fec=fec, locked=locked, ambiguous=ambiguous)
    est = [rec(capi.FEC34), rec(capi.FEC12), rec(-1, 0), rec(capi.FEC78), rec(capi.FEC12), rec(capi.FEC56, 0), rec(capi.FEC23, 1, 1), rec(capi.FEC34)]
    groups, left = capi.group_by_fec(est)
    assert groups == [(capi.FEC12, [1, 4]), (capi.FEC34, [0, 7]), (capi.FEC78, [3])] and left == [2, 5, 6]
    assert capi.group_by_fec([]) == ([], [])
