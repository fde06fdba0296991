"""leansdr_amd/tolerance.py — THE tolerance of the time-tiled (throughput) receiver, stated once.

LSDR_RX_TILED (cstln_receiver.hip) is not bit-exact: every tile but the first re-acquires symbol timing and carrier phase
during its warm-up, so its loop state differs from the reference's serial trajectory (sdr.h:772-916) by loop noise.  What is
promised — and asserted with these numbers by tests/test_gpu_rx_tiled.py, tests/test_gpu_rx_u8.py, bench.py's `verified`
objects and tools/rx_tol_report.py — against the oracle's exact serial receiver started from the same loop state, on a locked
QPSK stream at the bench condition (Es/N0 = 20 dB in leansdr_amd.synth's definition):

  count            exactly the same number of soft symbols for the same consumed input
  first tile       bit-exact (it continues from the carried state with the reference's arithmetic)
  decisions        >= min_equal_decisions identical `symbol` fields
  cost, mean       mean |Δcost| <= max_mean_abs_dcost        (cost = the soft symbol's int16 confidence, |cost| <= COST_MAX = 11236)
  cost, p99        99th percentile of |Δcost| <= max_p99_abs_dcost
  cost, max        no single symbol further than max_abs_dcost from the serial receiver's
  seams            no seam left unreconciled (bad_seams == 0)
  reports          signal-strength report and carried AGC within ss_rtol, MER report within mer_atol_db

LOW_SNR holds the same bounds for the 10–12 dB checks (the loops' own noise is larger there; a few seams may stay
unrepaired — they cost a handful of symbols that the FEC corrects, and are counted).

Which constellations: the tolerance is stated and tested for BPSK (TOL_BPSK), QPSK (TOL, LOW_SNR) and 8PSK (TOL_PSK8) —
tests/test_gpu_rx_tiled_constellations.py, on streams whose carrier phase walks through every rotation of the constellation.
For 16-ary and denser constellations the per-tile re-acquisition from phase = 0 is not reliable even with the reference's own
arithmetic: restated with the serial oracle alone (tests/test_oracle_rx_tile_emulation.py;
profiles/rx_tiled_constellations/emulation.txt), 1024-sample tiles after 1024 samples of warm-up at 26 dB give 99.45 % of the
serial receiver's decisions for 16QAM 3/4 and 92.4 % for 16APSK 3/4 (3 of 22 tiles below 95 %, the worst at 33 %: the 12-point
ring false-locks).  Nothing is refused, but those constellations should use the serial mode.
"""
import os

import numpy as np

COST_MAX = 11236          # largest |cost| of the QPSK table (cstln_lut<256>, sdr.h:529-560)
COST_MAX_BPSK = 31799     # largest |cost| of the BPSK 1/2 table
COST_MAX_PSK8 = 7943      # largest |cost| of the 8PSK 2/3 table

# How the bounds were set (round 4): every comparison made by the gpu tests and by bench.py's verification was logged
# (LSDR_TOL_LOG, below; profiles/r04_tolerance.txt) and each bound is 1.5 × the largest figure seen, rounded up —
#   TOL      bench geometry (256-sample tiles after 256 of warm-up) on the C2 chain, loops settled: mean |Δcost| 185–219,
#            p99 848, max 1908–2332; the other tile geometries of tests/test_gpu_rx_tiled.py: 137–155 / 424 / 636–1060; cu8 and
#            fir_sampler runs: 74–78 / 212 / 636; identical decisions everywhere, no unreconciled seam
#   LOW_SNR  C2 chain at 12 / 10 dB: mean 248 / 331, p99 1060 / 1696, max 3392 / 7632 (a flipped decision moves a cost by up to
#            2·COST_MAX; 0.07 % of the decisions differ at 10 dB), 4 unreconciled seams in 1036 tiles at 10 dB
# so a regression that doubles any error figure fails.
#
# Why these bounds are harmless where it matters — near the FEC threshold — is not argued from the per-symbol figures but MEASURED: the
# reference's sensitivity benchmark (test/leandvb_bench.sh) with the tiled receiver, the blk filter, the scan and fused notch and
# lsdr_capture_batch next to the reference binaries on the same deterministic inputs, profiles/r06_sensitivity/ (round 6, the final code):
# VBER within 3e-5 of the reference's on every series down to the SNR where the reference itself loses lock, transport stream byte-identical
# from 13 dB up at 1.2 sps, and never fewer packets out.  A loop-reconvergence error of 31 % of COST_MAX on single symbols (max_abs_dcost) is
# the loops' own noise at the seam, not a bias: it does not show in the decoded stream.  tests/test_gpu_sensitivity.py re-runs points of those
# curves on every -m gpu run.
#
# freq_atol (cycles per sample) belongs to lsdr_capture_batch's signal reports (lsdr_capture_reports_set: FREQ / SS / MER per capture, the
# serial receiver's sdr.h:857-913) and was set by the same rule: tests/test_gpu_capture_batch_reports.py logs |FREQ − the oracle's| at every
# compared instant (LSDR_REPORTS_LOG; profiles/capture_batch_reports/deviation.txt) — default engine at noise 7.5 (TOL): at most 1.13e-5;
# Viterbi engine at noise 18 (LOW_SNR), whose PLL is six times slower and has not fully converged where a tile body starts: at most 1.97e-5,
# seen under a carrier offset of 2e-4.  The serial FREQ itself jitters by about 6e-5 from instant to instant at noise 7.5: the tiles follow
# it.  Both bounds are below half the carrier offset that test applies (1e-4 / 2e-4), so a report of constant 0 fails.  The reports' SS and
# MER use ss_rtol / mer_atol_db as they stand (largest seen: 0.8 % and 0.23 dB under TOL, 1.1 % and 0.20 dB under LOW_SNR).
#
# freq_atol_tuned: the same reports of a capture that is TUNED (lsdr_capture_each: set_freq(tune), the carrier at tune), by the same rule from
# tests/test_gpu_capture_each.py's log (profiles/capture_batch_each/deviation.txt: tunes 0, ±1e-3 and 3e-3 of one capture, both engines).
# The default engine stays inside freq_atol tuned or not (at most 9.08e-6), so TOL has no tuned entry.  The Viterbi engine at noise 18 holds
# 6.84e-6 untuned and 3.55e-5 at a tune of −1e-3 — a single instant; the means agree to 2e-6 and the serial FREQ jitters more than that
# between instants.  SS and MER stay far inside their bounds tuned as well (0.9 %, 0.21 dB).
#
# TOL_BPSK / TOL_PSK8 (the tiled mode beyond QPSK): NOT from the GPU's output but from the tile algorithm restated with the serial oracle alone
# (tests/rx_tiled_common.emulate_tiles: every tile restarts the reference's loops from mu = phase = 0 one warm-up early; figures against the
# serial oracle in profiles/rx_tiled_constellations/emulation.txt, written by tests/test_oracle_rx_tile_emulation.py, which also asserts that the
# bounds below follow from them).  Streams of tests/rx_tiled_common.CASES, geometries (1024, 1024) / (512, 512) / (256, 1024); each bound is
# 1.5 × the worst of the three, rounded up —
#   TOL_BPSK  BPSK 1/2 at 12 dB: mean |Δcost| 876 / 978 / 908, p99 2215 / 2544 / 2332, max 8766 / 9047 / 8783 (|cost| <= COST_MAX_BPSK),
#             identical decisions 1 / 0.999866 / 0.999955
#   TOL_PSK8  8PSK 2/3 at 26 dB: mean 70 / 122 / 84, p99 236 / 367 / 265, max 536 / 618 / 428 (|cost| <= COST_MAX_PSK8),
#             identical decisions 0.999950 / 0.999749 / 1
# The QPSK stream of those tests (table slicer; carrier offset with allow_drift) runs under TOL itself: emulated mean 71 / 115 / 73, p99 212 / 424 /
# 212, max 424 / 1484 (2544 with the offset) / 424, every decision identical.  SS, MER and the seams are held to TOL's entries as they stand
# (the wrong estimator branch for BPSK would move MER by about 3 dB); freq_atol is carried over unmeasured: the capture batch decodes QPSK only.
TOL = dict(
    min_equal_decisions=0.9995,
    max_mean_abs_dcost=330,       # 1.5 × 219
    max_p99_abs_dcost=1300,       # 1.5 × 848
    max_abs_dcost=3500,           # 1.5 × 2332
    max_bad_seams=0,
    ss_rtol=0.02,
    mer_atol_db=1.0,
    freq_atol=2e-5,               # 1.5 × 1.13e-5: the capture batch's FREQ reports, default engine (see above)
)

LOW_SNR = dict(
    min_equal_decisions=0.998,    # measured 0.99934 at 10 dB
    max_mean_abs_dcost=500,       # 1.5 × 331
    max_p99_abs_dcost=2600,       # 1.5 × 1696
    max_abs_dcost=11500,          # 1.5 × 7632
    max_bad_seams_per_1000_tiles=8,   # measured 3.9 at 10 dB, 0 at 12 dB
    ss_rtol=0.05,
    mer_atol_db=1.0,
    freq_atol=3e-5,               # 1.5 × 1.97e-5: the capture batch's FREQ reports, Viterbi engine at noise 18 (see above)
    freq_atol_tuned=5.33e-5,      # 1.5 × 3.55e-5: … of a tuned capture (see above)
)

TOL_BPSK = dict(TOL,
    min_equal_decisions=0.99979,  # 1 − 1.5 × (1 − 0.999866)
    max_mean_abs_dcost=1470,      # 1.5 × 978.4
    max_p99_abs_dcost=3820,       # 1.5 × 2544
    max_abs_dcost=13600,          # 1.5 × 9047
)

TOL_PSK8 = dict(TOL,
    min_equal_decisions=0.99962,  # 1 − 1.5 × (1 − 0.999749)
    max_mean_abs_dcost=185,       # 1.5 × 121.7
    max_p99_abs_dcost=555,        # 1.5 × 367.3
    max_abs_dcost=930,            # 1.5 × 618
)

_TOL_NAMES = ((TOL, "TOL"), (TOL_BPSK, "TOL_BPSK"), (TOL_PSK8, "TOL_PSK8"))


def check_tiled(sym, ref_sym, stats=None, first_exact=0, tol=None):
    """Compare a tiled run's soft symbols with the serial reference's under `tol` (default TOL).  Returns a report dict with
    every measured figure and `pass`.  first_exact: number of leading symbols that must be bit-identical (inside tile 0)."""
    tol = TOL if tol is None else tol
    rep = dict(symbols=int(len(sym)), symbols_ref=int(len(ref_sym)), count_equal=bool(len(sym) == len(ref_sym)))
    ok = rep["count_equal"]
    if ok:
        same = float((sym["symbol"] == ref_sym["symbol"]).mean()) if len(sym) else 1.0
        dc = np.abs(sym["cost"].astype(np.int64) - ref_sym["cost"].astype(np.int64))
        rep.update(equal_decisions=round(same, 6), mean_abs_dcost=round(float(dc.mean()), 2) if len(dc) else 0.0,
                   p99_abs_dcost=float(np.percentile(dc, 99)) if len(dc) else 0.0, max_abs_dcost=int(dc.max()) if len(dc) else 0)
        ok = (same >= tol["min_equal_decisions"] and rep["mean_abs_dcost"] <= tol["max_mean_abs_dcost"]
              and rep["p99_abs_dcost"] <= tol["max_p99_abs_dcost"] and rep["max_abs_dcost"] <= tol["max_abs_dcost"])
        if first_exact:
            rep["first_tile_bit_exact"] = bool(sym["cost"][:first_exact].tobytes() == ref_sym["cost"][:first_exact].tobytes()
                                               and sym["symbol"][:first_exact].tobytes() == ref_sym["symbol"][:first_exact].tobytes())
            ok = ok and rep["first_tile_bit_exact"]
    if stats is not None:
        rep["tiles"] = int(stats["tiles"]); rep["bad_seams"] = int(stats["bad_seams"])
        rep["seams_repaired"] = int(stats["dup"]) + int(stats["miss"])
        if "max_bad_seams" in tol:
            ok = ok and rep["bad_seams"] <= tol["max_bad_seams"]
        else:
            ok = ok and rep["bad_seams"] * 1000 <= tol["max_bad_seams_per_1000_tiles"] * max(1, rep["tiles"])
    rep["pass"] = bool(ok)
    log = os.environ.get("LSDR_TOL_LOG")          # every comparison's measured figures, one JSON line each (how the bounds above were set)
    if log:
        import json
        with open(log, "a") as f:
            f.write(json.dumps(dict(rep, tol=next((n for t, n in _TOL_NAMES if tol is t), "LOW_SNR"), where=os.environ.get("PYTEST_CURRENT_TEST", ""))) + "\n")
    return rep
