"""Shared helpers of the spectrum batch's tests (lsdr_spectrum_batch, include/lsdr_hip.h): the row/block rule restated — a test oracle, never
imported by the product — and the captures the tests measure.

The rule (cnr_fft::run and spectrum::run, sdr.h:1292-1301 and 1362-1371): `phase` grows by nfft per whole block of nfft samples; the block
with which it reaches `decimation` is fetched and decimation is subtracted.  With decimation >= nfft at most one row per block, so row m
(1-based) is taken from block ceil(m·decimation/nfft) − 1, J = n // nfft whole blocks give (J·nfft) // decimation rows, and J·nfft samples
are consumed."""
import functools

import numpy as np
import resample_common as rc

DECIMATIONS = {1024: (1024, 1025, 3000, 2048, 5 * 1024 - 7), 4096: (4096, 4097, 8192, 5 * 4096 - 7), 64: (64, 65, 128, 5 * 64 - 7)}


def rows_of(n, nfft, decimation):
    """(rows, consumed) of a capture of n samples."""
    assert decimation >= nfft
    blocks = int(n) // nfft
    return (blocks * nfft) // decimation, blocks * nfft


def block_of_row(m, nfft, decimation):
    """The 0-based block row m (1-based) is taken from."""
    return -(-(m * decimation) // nfft) - 1


def fetched_blocks(n, nfft, decimation):
    """The blocks run()'s phase counter fetches, by running the counter."""
    phase, out = 0, []
    for j in range(int(n) // nfft):
        phase += nfft
        if phase >= decimation:
            phase -= decimation
            out.append(j)
    return out


def lengths_around(nfft, decimation):
    """Lengths at which the counts change: 0, around every multiple of nfft up to a few rows, around the samples that complete a row."""
    out = {0, nfft - 1, nfft, nfft + 1}
    for k in range(1, 14):
        out |= {k * nfft - 1, k * nfft, k * nfft + 17}
    for m in range(1, 4):
        edge = (block_of_row(m, nfft, decimation) + 1) * nfft
        out |= {edge - 1, edge, edge + 1}
    return sorted(out)


@functools.lru_cache(maxsize=None)
def capture4(noise, seed=11):
    """A cu8 capture at 4 samples per symbol, 16 packets (104525 samples: 25 blocks of 4096)."""
    from leansdr_amd import synth_dvbs
    iq, _ = synth_dvbs.capture_u8(n_packets=16, sps_num=4, sps_den=1, seed=seed, noise_std=noise)
    return np.ascontiguousarray(iq)


def formats_of(u8):
    """resample_common.formats_of: the cu8 items as cs8, cu16, cs16 (in_scale 2^-8) and cf32."""
    return rc.formats_of(u8)
