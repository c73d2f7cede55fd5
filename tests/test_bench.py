"""bench.py --dump-outputs: the fields the last timed step left, written as float64 .npy files; the same arguments give the same
files (the spin-up, warm-up and timed step counts follow from the arguments alone), and a larger output is a fixed sample."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, outdir):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "OCNHIP_LIB"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(outdir)], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    files = {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(os.path.join(str(outdir), "*.npy"))}
    return rec, files


def check_two_runs(args, tmp_path, names, steps):
    rec, a = run_bench(args, tmp_path / "a")
    _, b = run_bench(args, tmp_path / "b")
    assert rec["steps"] == steps and rec["ms_per_step"] > 0
    assert set(a) == set(names) and set(b) == set(names)
    assert sum(os.path.getsize(p) for p in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 64 << 20
    for n in names:
        assert a[n].dtype == np.float64 and np.isfinite(a[n]).all(), n
        assert np.array_equal(a[n], b[n]), n
    return a


@pytest.mark.parametrize("config,names", [("2", ("u", "v", "w")), ("5", ("u", "v", "w", "T", "S", "eta"))])
def test_dump_outputs_repeat_hostemu(config, names, backend, tmp_path):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    a = check_two_runs(["--config", config, "--gpus", "1", "--rehearse-hostemu", "--steps", "2", "--warmup", "1"], tmp_path, names, 2)
    if config == "2":
        assert a["u"].shape == (16, 16, 8)


@pytest.mark.gpu
def test_dump_outputs_repeat_gpu(tmp_path):
    a = check_two_runs(["--gpus", "1", "--size", "32", "32", "32", "--steps", "3", "--warmup", "2", "--no-cpu-baseline"], tmp_path,
                       ("u", "v", "w"), 3)
    assert a["u"].shape == (32, 32, 32) and np.abs(a["u"]).max() > 0


def test_dump_outputs_sample_larger_fields(monkeypatch, tmp_path):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    rng = np.random.default_rng(5)
    fields = {"u": rng.random((64, 64, 64)), "w": rng.random((64, 64, 65)), "eta": rng.random((64, 64, 1))}
    bench.dump_outputs(str(tmp_path), fields, 0, 1)
    assert sum(os.path.getsize(p) for p in glob.glob(str(tmp_path / "*.npy"))) <= 1 << 20
    eta = np.load(tmp_path / "eta.npy")
    assert eta.dtype == np.float64 and np.array_equal(eta, fields["eta"])     # small enough to stay whole
    for n in ("u", "w"):
        s = np.load(tmp_path / f"{n}.npy")
        idx = np.sort(np.random.default_rng(0).choice(fields[n].size, s.size, replace=False))
        assert s.ndim == 1 and s.dtype == np.float64 and np.array_equal(s, fields[n].ravel(order="F")[idx]), n
    fields = {"u": np.zeros((8, 8, 8), dtype=np.float32)}                          # fits: whole array, float64
    bench.dump_outputs(str(tmp_path / "small"), fields, 1, 2)
    s = np.load(tmp_path / "small" / "u_rank1.npy")
    assert s.shape == (8, 8, 8) and s.dtype == np.float64
