"""bench.py's command line: ``--dump-outputs`` (what the last timed step returned, comparable between
runs and builds), ``--steps`` / ``ms_per_step``, and ``--full`` (the extras stay out of a plain run)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_KEYS = ("rfft2_720x1440_us", "fno_block_720x1440_bf16_us", "native_export_samples_per_s", "bf16_samples_per_s")


def _bench(*args):
    # a CPU-tier test: hide any GPU, as the torchrun harness tests do
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--tiny", "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_same_from_run_to_run(tmp_path):
    d1 = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    d2 = _bench("--steps", "2", "--warmup", "0", "--full", "--dump-outputs", str(tmp_path / "b"))
    assert d1["steps"] == 3 and d2["steps"] == 2 and d1["ms_per_step"] > 0 and d2["ms_per_step"] > 0
    for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert k in d1
    assert not any(k in d1 for k in EXTRA_KEYS)  # a plain run measures the headline only
    assert os.listdir(tmp_path / "a") == ["output.npy"]
    a, b = np.load(tmp_path / "a" / "output.npy"), np.load(tmp_path / "b" / "output.npy")
    assert a.dtype == np.float32 and a.shape == (2, 4, 48, 96)  # the tiny model's whole output
    assert d1["dumped_outputs"]["output"] == {"shape": [2, 4, 48, 96], "dtype": "float32", "sampled": False}
    assert np.isfinite(a).all() and a.std() > 0
    assert np.array_equal(a, b)  # seeded weights and inputs: the same output whatever the step count


def test_dump_outputs_samples_a_large_output(tmp_path):
    spec = importlib.util.spec_from_file_location("bench_main", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # bench/ is a package: load the script by path
    n = mod.DUMP_WHOLE_BYTES // 4 + 1  # one element past what is written whole
    t = (torch.arange(n, dtype=torch.int32) % 65521).to(torch.bfloat16).view(1, n)
    small = torch.arange(6, dtype=torch.float64).view(2, 3)
    note = mod.dump_outputs(str(tmp_path), {"big": t, "small": small})
    big = np.load(tmp_path / "big.npy")
    assert note["big"] == {"shape": [mod.DUMP_SAMPLE], "dtype": "float32", "sampled": True}
    assert big.dtype == np.float32 and big.nbytes + small.numel() * 8 <= 64 << 20
    idx = torch.randint(0, n, (mod.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0))
    assert np.array_equal(big, t.view(-1)[idx].float().numpy())  # the documented positions, in order
    assert idx.min() < n // 100 and idx.max() > n - n // 100  # spread over the whole output
    s = np.load(tmp_path / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small.numpy())
