"""bench.py's command line on the CPU (gloo rehearsal, gpt2-tiny): ``--steps`` sets the number of timed
steps, ``ms_per_step`` is the time of one of them, ``--dump-outputs`` writes the last timed step's
loss as a float32 .npy that is identical from run to run, and ``--full`` is accepted."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(tmp_path, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(TMPDIR=str(tmp_path), OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--device", "cpu", "--model",
                        "gpt2-tiny", "--warmup", "1", "--batch", "2", "--seq", "64", *extra],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(recs) == 1, r.stdout
    return recs[0]


def test_bench_dump_outputs_and_full_cpu(tmp_path):
    a = _bench(tmp_path, "--steps", "3", "--dump-outputs", str(tmp_path / "a"))
    b = _bench(tmp_path, "--steps", "2", "--full", "--dump-outputs", str(tmp_path / "b"))
    c = _bench(tmp_path, "--steps", "3", "--full", "--dump-outputs", str(tmp_path / "c"))
    for rec, steps in ((a, 3), (b, 2), (c, 3)):
        assert all(k in rec for k in HEADLINE_KEYS), rec
        assert rec["steps"] == steps and rec["unit"] == "tokens/s" and rec["higher_is_better"] is True
        # value is tokens per second of the timed steps: batch * seq tokens every ms_per_step
        assert rec["ms_per_step"] > 0 and abs(rec["value"] - 2 * 64 / (rec["ms_per_step"] / 1000)) / rec["value"] < 0.01
    la, lb, lc = (np.load(tmp_path / d / "loss.npy") for d in "abc")
    for d in "abc":
        assert os.listdir(tmp_path / d) == ["loss.npy"]
    assert la.dtype == np.float32 and la.shape == (1,) and np.isfinite(la).all()
    assert abs(float(la[0]) - a["final_loss"]) < 1e-3  # (the record rounds to 4 places)
    assert np.array_equal(la, lc)  # same arguments: same inputs, same output (CPU fp32 is deterministic)
    assert not np.array_equal(la, lb)  # one step fewer: the dump is the LAST timed step's loss
