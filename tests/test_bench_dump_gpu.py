"""`bench.py --dump-outputs DIR` on the headline path (one captured hipGraph per step, training-mode noise): `--steps` timed steps run,
`ms_per_step` is their mean, the dumped loss is the last timed step's, and two runs with the same arguments dump the same bits (what
lets two builds be compared output for output).  Every run is a FRESH child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    env = dict(os.environ, PYTHONPATH=ROOT, CLC_BENCH_LOSS_TRACE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CLC_FORCE_COLLECTIVES", "CLC_FORCE_SPLIT_GRAPHS", "CLC_BENCH_EVAL_ROUNDING"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
                        "--no-roofline", "--no-parity", "--no-reduced", "--no-reference-loop", "--no-cpu-baseline", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=360, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_dump_outputs_are_the_last_timed_step_and_reproducible(dev, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ra = _bench(a)
    assert ra["steps"] == 3 and len(ra["config"]["loss_trace"]) == 1 + 3          # one warm-up step, three timed ones
    assert ra["ms_per_step"] > 0 and abs(ra["value"] * ra["ms_per_step"] - 4 * 1e3) <= 1e-6 * 4e3
    names = sorted(os.listdir(a))
    assert {"loss.npy", "bpp_loss.npy", "mse_loss.npy", "aux_loss.npy", "params.npy"} <= set(names)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in names) <= 64 << 20
    arrs = {f: np.load(os.path.join(a, f)) for f in names}
    assert all(v.dtype in (np.float32, np.float64) for v in arrs.values())
    assert float(arrs["loss.npy"]) == ra["config"]["loss_trace"][-1] == ra["config"]["final_loss"]
    assert np.isfinite(arrs["params.npy"]).all() and arrs["params.npy"].size > 0
    rb = _bench(b)
    assert ra["config"]["loss_trace"] == rb["config"]["loss_trace"]
    for f in names:
        assert np.array_equal(arrs[f], np.load(os.path.join(b, f))), f"{f} differs between two runs with the same arguments"


def test_plain_run_prints_the_headline_and_runs_no_other_leg(dev):
    """Without --full the run stops after the timed steps: the headline fields and `config`, none of the legs' objects."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CLC_FORCE_COLLECTIVES", "CLC_FORCE_SPLIT_GRAPHS", "CLC_BENCH_EVAL_ROUNDING", "CLC_BENCH_LOSS_TRACE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4"],
                       capture_output=True, text=True, timeout=360, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    rep = json.loads(lines[0])
    assert rep["unit"] == "images/sec" and rep["higher_is_better"] is True and rep["dtype"] == "f32" and rep["steps"] == 2
    assert rep["ms_per_step"] > 0 and abs(rep["value"] * rep["ms_per_step"] - 4 * 1e3) <= 1e-6 * 4e3
    assert not {"roofline", "parity", "codec", "reduced_precision", "reference_loop", "cpu_baseline"} & set(rep), sorted(rep)
