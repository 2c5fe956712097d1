"""bench.py --dump-outputs / --full: a plain run times the steps and nothing else; the dump holds
what the last timed step computed, as float .npy files within the byte budget, and the same
arguments give the same step in every process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("R", "t", "pred_t", "inliers", "xyz")


def test_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    import bench
    g = torch.Generator().manual_seed(0)
    outs = {"R": torch.randn(4, 3, 3, generator=g), "inliers": torch.arange(4, dtype=torch.int32),
            "ext": torch.randn(4, 3, generator=g, dtype=torch.float64), "xyz": torch.randn(4, 3, 32, 32, generator=g)}
    bench.dump_outputs(str(tmp_path / "a"), outs)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in outs}
    assert {k: v.dtype for k, v in got.items()} == {"R": np.float32, "inliers": np.float32, "ext": np.float64,
                                                    "xyz": np.float32}
    for k, v in outs.items():
        assert got[k].shape == tuple(v.shape) and np.array_equal(got[k], v.numpy().astype(got[k].dtype))

    # over the budget: the large array becomes a fixed sample of its flat elements, the small ones stay whole
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), outs)
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in outs}
    assert sum(v.nbytes for v in b.values()) <= 4096
    assert all(np.array_equal(b[k], got[k]) for k in ("R", "inliers", "ext"))
    assert b["xyz"].shape == (256,) and np.isin(b["xyz"], got["xyz"]).all()
    assert np.array_equal(b["xyz"], np.load(tmp_path / "c" / "xyz.npy"))


def test_breakdown_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--breakdown", "x.json"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(dev, tmp_path, capsys, monkeypatch):
    """A plain run in a fresh process and the same run in this one: no roofline / CPU leg in the
    result line, ms_per_step and value agree with each other, every output is written and is
    identical between the two processes bit for bit."""
    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64", "--points", "256"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv + ["--dump-outputs", str(tmp_path / "a")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "crops/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["config"]["graph"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["accuracy"] is None
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01

    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv + ["--dump-outputs", str(tmp_path / "b")])
    bench.main()
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["roofline"] is None
    shapes = {"R": (2, 3, 3), "t": (2, 3), "pred_t": (2, 3), "inliers": (2,), "xyz": (2, 3, 64, 64)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in NAMES)
    for k in NAMES:
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == shapes[k] and np.isfinite(a).all(), k
        assert np.array_equal(a, b), k
    assert np.abs(np.load(tmp_path / "a" / "xyz.npy")).max() > 0
