"""`python3 bench.py --gpus N` invoked bare (the driver's N = 1 command shape; no torch.distributed.run): the script starts its
own ranks — fresh child processes, never an exec of a process that touched the GPU — or says plainly why it cannot."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_bare_multi_gpu_command_without_a_gpu_says_so():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=_env())
    assert r.returncode == 1, (r.returncode, r.stderr[-500:])
    assert "needs 2 MI355X devices" in r.stderr and "torch.distributed.run" not in r.stderr
    assert r.stdout.strip() == ""


def test_mismatched_world_size_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=300,
                       env=_env(WORLD_SIZE="1", RANK="0"))
    assert r.returncode == 2 and "WORLD_SIZE=1" in r.stderr


@pytest.mark.gpu
def test_bare_multi_gpu_command_rehearsed_on_one_device(gpu):
    """Two ranks on cuda:0 through the bare command (gloo carries the bootstrap; the collectives are the C ABI's one-shot
    kernels): rank 0's line comes back through the parent, n_gpus = 2."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--prefill", "128",
                        "--decode", "4"], capture_output=True, text=True, timeout=900, env=_env(LFAMD_DIST_BACKEND="gloo"))
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["value"] > 0 and "invalid" not in d


def test_dump_sample_is_fixed():
    """--dump-outputs samples an output larger than its share at indices that depend on the file name and size alone."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    assert bench.dump_sample_index("decode.output", 1000, 1000) is None
    a = bench.dump_sample_index("prefill.output", 5_000_000, 4096)
    b = bench.dump_sample_index("prefill.output", 5_000_000, 4096)
    assert np.array_equal(a, b) and len(np.unique(a)) == 4096 and (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < 5_000_000
    assert not np.array_equal(a, bench.dump_sample_index("prefill.blk.31.ffn_up", 5_000_000, 4096))


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(gpu, tmp_path):
    """A plain run: the line holds ms_per_step over the steps asked for and none of the --full legs; --dump-outputs writes the
    last step's outputs as float32 .npy files under 64 MB in all, and a second run with the same arguments writes the same values."""
    import numpy as np
    runs = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--prefill", "128",
                            "--decode", "4", "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=600, env=_env())
        assert r.returncode == 0, r.stderr[-3000:]
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and "roofline" not in d and d["cpu_baseline"] is None
        runs.append({f: np.load(tmp_path / tag / f) for f in sorted(os.listdir(tmp_path / tag))})
    a, b = runs
    assert "decode.output.npy" in a and "prefill.blk.31.ffn_down.npy" in a and a.keys() == b.keys()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= 64 << 20
    for f in a:
        assert a[f].dtype == np.float32 and np.isfinite(a[f]).all() and np.abs(a[f]).max() > 0, f
        assert np.array_equal(a[f], b[f]), f
