"""bench.py's plain run and its options: `--steps` sets the timed steps, `--dump-outputs DIR` writes what the last
timed step returned (float32 .npy, logical NCHW order), `--full` adds the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config"}


def _bench():
    import bench
    return bench


def test_parse_defaults_and_steps_floor():
    bench = _bench()
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d", "--steps", "3"])
    assert a.full and a.dump_outputs == "d" and a.steps == 3
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_writes_float32_in_logical_order(tmp_path):
    bench = _bench()
    x = torch.randn(2, 6, 3, 5).contiguous(memory_format=torch.channels_last)
    bench.dump_outputs(str(tmp_path), {"out": x, "grad_x": x.to(torch.bfloat16)})
    out, gx = np.load(tmp_path / "out.npy"), np.load(tmp_path / "grad_x.npy")
    assert out.dtype == np.float32 and gx.dtype == np.float32
    assert np.array_equal(out, x.numpy()) and np.array_equal(gx, x.to(torch.bfloat16).float().numpy())


def test_dump_outputs_samples_the_same_elements_above_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 400)
    x = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"out": x, "grad_x": -x})
    a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    g = np.load(tmp_path / "a" / "grad_x.npy")
    assert 4 * (a.size + g.size) <= 400 and a.size > 0
    assert np.array_equal(a, b) and np.array_equal(g, -a)
    assert np.all(np.diff(a) > 0)         # distinct flat indices, in order


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    """A plain run prints the headline fields only, for exactly --steps steps; its dump is the module's out / grad_x on
    the seeded inputs, checked against the CPU oracle."""
    import oracle
    bench = _bench()
    argv = ["--steps", "3", "--warmup", "1", "--batch", "4", "--channels", "64"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv, "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert set(res) == HEADLINE_KEYS
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["unit"] == "Mpixels/s"
    args = bench.parse(argv)
    w = bench.Workload(args, torch.device("cuda", 0), 0, sets=1)
    x, go = w.x[0].detach().cpu().numpy(), w.go[0].cpu().numpy()
    ctor = bench.module_ctor(args)
    ref_out, ref_gx = oracle.forward(x, **ctor), oracle.backward(x, go, **ctor)
    out, gx = np.load(tmp_path / "out.npy"), np.load(tmp_path / "grad_x.npy")
    assert out.shape == ref_out.shape and gx.shape == ref_gx.shape
    assert np.abs(out - ref_out).max() / np.abs(ref_out).max() <= 1e-5
    assert np.abs(gx - ref_gx).max() / np.abs(ref_gx).max() <= 1e-5
