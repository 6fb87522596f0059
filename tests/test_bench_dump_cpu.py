"""`bench.py --dump-outputs DIR`: what the last timed step returned (float64 scalars) and the parameters it left (float32, a fixed seeded
sample when they exceed the 64 MB budget) as DIR/<name>.npy; and `--steps` below 1 is refused (it is the number of timed steps)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _total_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_small_model_writes_every_parameter(tmp_path):
    import bench

    m = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))
    out = {"loss": torch.tensor(1.25), "bpp_loss": torch.tensor(0.5), "aux_loss": torch.tensor(3.0)}
    files = bench.dump_outputs(str(tmp_path), out, m)
    assert set(files) == {"loss", "bpp_loss", "aux_loss", "params"}
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in files)
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float64 and loss.shape == () and float(loss) == 1.25
    p = np.load(tmp_path / "params.npy")
    want = torch.cat([q.detach().reshape(-1) for q in m.parameters()]).numpy()
    assert p.dtype == np.float32 and np.array_equal(p, want)


def test_dump_large_model_is_a_fixed_sample_within_budget(tmp_path):
    import bench

    n = bench.DUMP_BUDGET_BYTES // 4 + 1000          # one parameter just over the budget
    m = torch.nn.Module()
    m.w = torch.nn.Parameter(torch.arange(n, dtype=torch.float32))
    out = {"loss": torch.tensor(2.0)}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), out, m)
    bench.dump_outputs(str(b), out, m)
    assert _total_bytes(a) <= bench.DUMP_BUDGET_BYTES
    pa, pb = np.load(a / "params.npy"), np.load(b / "params.npy")
    assert pa.dtype == np.float32 and pa.shape == (bench.DUMP_PARAM_SAMPLE,)
    assert np.array_equal(pa, pb)                      # same positions every run
    # the values of arange are the positions (exact in float32 below 2**24): ascending, no repeats, spread over the whole parameter
    assert np.all(np.diff(pa) >= 0) and pa[0] >= 0 and pa[-1] >= n - 3 * n // bench.DUMP_PARAM_SAMPLE
    exact = pa[pa < 2 ** 24]
    assert len(exact) > 0.99 * bench.DUMP_PARAM_SAMPLE and np.all(np.diff(exact) > 0)


def test_steps_below_one_is_refused():
    e = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120, env=e, cwd=ROOT)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr
