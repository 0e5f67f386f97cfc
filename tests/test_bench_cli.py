"""bench.py's launch contract, checked without a GPU: `--gpus N` with no launcher around it starts the
ranks itself and REFUSES (non-zero exit, a message, no JSON line) when fewer than N devices are
visible -- it never prints an n_gpus: 1 line for an N-GPU request (missing #1)."""
import os
import subprocess
import sys

import pytest

from conftest import REPO


def _run(*args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], env=env, capture_output=True,
                          text=True, timeout=timeout)


def _visible():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def test_more_gpus_than_visible_is_refused_loudly():
    n = _visible() + 1 if _visible() else 2
    r = _run("--gpus", str(n), "--steps", "2", "--warmup", "1")
    assert r.returncode != 0
    assert "refusing to run" in r.stderr and f"--gpus {n}" in r.stderr
    assert r.stdout.strip() == ""                        # no JSON line of a smaller job


def test_world_size_mismatch_is_refused():
    r = _run("--gpus", "4", env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)
    assert "n_gpus" not in r.stdout


def test_no_gpu_means_no_number():
    if _visible():
        pytest.skip("a GPU is visible")
    r = _run("--gpus", "1", "--steps", "2", "--warmup", "1")
    assert r.returncode != 0 and "no CPU fallback" in (r.stderr + r.stdout)
    assert "value" not in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--force-shard", "--n", "2048")])
def test_exactly_one_json_line_on_stdout(extra):
    """The contract: rank 0 prints ONE JSON line.  RCCL writes its version banner to the process's
    stdout as late as library teardown; bench.py keeps fd 1 parked on stderr so that nothing but the
    line arrives -- with the process group (and the RCCL communicator) of the sharded code path too."""
    import json
    r = _run("--full", "--steps", "2", "--warmup", "1", "--no-extras", "--no-cpu-baseline", *extra, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:2000]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["warmup"] == 1 and d["steps"] == 2 and d["n_gpus"] == 1
    assert d["roofline"]["bound"] == "mfma" and 0.2 < d["roofline"]["frac"] < 1.0


def test_steps_and_warmup_are_validated():
    r = _run("--steps", "0")
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""


def test_dump_rows_fit_the_budget_and_are_fixed():
    """--dump-outputs: all of C while it fits, else the same seeded sample of its rows on every call."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(REPO, "bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert B.dump_rows(1024, 1024, 1) is None
    for rows, n, world in ((4096, 4096, 1), (16384, 16384, 1), (2048, 16384, 8)):
        sel = B.dump_rows(rows, n, world)
        assert sel is not None and list(sel) == sorted(set(sel)) and 0 <= sel[0] and sel[-1] < rows
        assert world * len(sel) * n * 4 <= B.DUMP_BYTES < 64 << 20
        assert list(sel) == list(B.dump_rows(rows, n, world))


@pytest.mark.gpu
def test_a_plain_run_times_its_steps_and_dumps_the_last_c(tmp_path, mm):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one line with the headline keys and nothing measured
    beside them; K timed steps; DIR/c.npy = the timed kernel's C (a seeded row sample at N = 4096), bit-equal to the
    128x128-tile launch on the same seeded inputs recomputed here."""
    import json
    import time
    import numpy as np
    import torch
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(REPO, "bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    t0 = time.time()
    r = _run("--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:2000]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["metric"] == B.METRIC and d["unit"] == "GFLOPS" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert abs(d["value"] - 2.0 * 4096 ** 3 * 1e-9 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    for key in ("cold", "roofline", "cpu_baseline", "extras", "bit_equal_to_128x128_tile_launch"):
        assert key not in d, key
    assert time.time() - t0 < 120
    files = sorted(os.listdir(tmp_path))
    assert files == ["c.npy"]
    assert os.path.getsize(tmp_path / "c.npy") <= 64 << 20
    got = np.load(tmp_path / "c.npy")
    sel = B.dump_rows(4096, 4096, 1)
    assert got.dtype == np.float32 and got.shape == (len(sel), 4096)
    n, dev = 4096, torch.device("cuda", 0)
    a = torch.rand((n, n), device=dev, generator=torch.Generator(device=dev).manual_seed(1234)) * 2 - 1
    b = torch.rand((n, n), device=dev, generator=torch.Generator(device=dev).manual_seed(99)) * 2 - 1
    c = torch.empty((n, n), device=dev)
    mm.set_kernel("mfma_tiles")
    try:
        mm.sgemm(n, n, n, a.data_ptr(), n, b.data_ptr(), n, c.data_ptr(), n, False, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        mm.set_kernel("mfma")
    want = c[torch.as_tensor(sel, device=dev)].cpu().numpy()
    assert np.array_equal(got, want)
