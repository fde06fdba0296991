"""bench.py's command line on hardware, at a small geometry: a plain run reports the headline only (everything else is --full's),
and --dump-outputs writes the same arrays from run to run with the same arguments — buffer placement, which plays a number of
batches that depends on timing before the warm-up, included."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--batch-msamples", "16", "--batches-per-step", "2", "--steps", "2", "--warmup", "1"]


def _run(extra, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(LSDR_BENCH_ARENA_GIB="8", LSDR_BENCH_PLACEMENT="4", LSDR_BENCH_FULL=str(tmp_path / "bench_full.json"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_its_dump_repeats(tmp_path):
    dumps = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        j = _run(["--dump-outputs", str(d)], tmp_path)
        assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
        assert j["unit"] == "MS/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
        for extra in ("verified", "unplaced", "cpu_baseline"):
            assert extra not in j, extra
        assert list(j["summary"]) == ["headline_c2", "_cols"]
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert sorted(dumps[0]) == ["c0_decimated_sample.npy", "c0_soft_symbols.npy"]
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20
    sym = dumps[0]["c0_soft_symbols.npy"]
    assert sym.dtype == np.float32 and sym.ndim == 2 and sym.shape[1] == 2 and len(sym) > 100000
    assert set(np.unique(sym[:, 1]).tolist()) <= {0.0, 1.0, 2.0, 3.0}          # QPSK decisions
    for f in dumps[0]:
        assert dumps[0][f].dtype == np.float32 and np.array_equal(dumps[0][f], dumps[1][f]), f


def test_full_run_verifies_its_timed_output(tmp_path):
    j = _run(["--full", "--no-cpu", "--no-more"], tmp_path)
    assert j["verified"]["pass"] and j["verified"]["fir_bit_exact"]
    assert "unplaced" in j
