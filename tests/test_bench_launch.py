"""bench.py's multi-GPU launcher (the driver's `python bench.py --gpus N` form).

CPU: `--gpus N --launch-only` starts N worker processes, each joins a gloo process group, and
rank 0's line reports n_gpus = N with N distinct ranks in ranks_seen (the launcher and the
report, without the model).  A worker that fails ends the others and the parent's exit code is
non-zero.  GPU: one rank through the RCCL ("nccl") process group on the box's GPU, a short
N=2 @518 bench step, and its ranks_seen entry names the device."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _json_line(out: str):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _cpu_env():
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""  # keep the CPU test on gloo even where a GPU exists
    env["CUDA_VISIBLE_DEVICES"] = ""
    env.pop("WORLD_SIZE", None)
    return env


@pytest.mark.parametrize("n", [2, 3])
def test_launcher_spawns_n_ranks(n):
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--launch-only"], capture_output=True, text=True,
                       timeout=300, env=_cpu_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == n and line["backend"] == "gloo"
    assert sorted(s["rank"] for s in line["ranks_seen"]) == list(range(n))
    assert sorted(s["local_rank"] for s in line["ranks_seen"]) == list(range(n))


def test_launcher_single_process_default():
    r = subprocess.run([sys.executable, BENCH, "--launch-only"], capture_output=True, text=True, timeout=300,
                       env=_cpu_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 1 and line["backend"] is None


def test_launcher_propagates_failure():
    """Without a GPU and without --launch-only every worker must refuse (no CPU fallback of the HIP
    path); the parent returns non-zero and prints no bench line."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True,
                       text=True, timeout=300, env=_cpu_env(), cwd=REPO)
    assert r.returncode != 0
    assert "no ROCm GPU" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_dump_outputs_files(tmp_path):
    """bench.dump_outputs: one float32 <name>.npy per result key stacked over the views, ``images``
    (the same tensor as ``rgbs``) not written twice, a large array as a fixed seeded sample of its
    flattened elements, everything within DUMP_MAX_BYTES, and the same bytes on a second call."""
    import numpy as np
    import torch

    import bench
    g = torch.Generator().manual_seed(3)
    big = torch.rand(2, 1, 3, 1500, 1500, generator=g)  # 54 MB as float32: over its third of the 64 MB
    results = [{"extrinsic": torch.rand(1, 3, 4, generator=g).double(), "cam_tokens": torch.rand(1, 8, generator=g).bfloat16(),
                "rgbs": big[i], "images": big[i]} for i in range(2)]
    bench.dump_outputs(str(tmp_path / "a"), results)
    bench.dump_outputs(str(tmp_path / "b"), results)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["cam_tokens.npy", "extrinsic.npy", "rgbs.npy"]
    arrs = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float32 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= bench.DUMP_MAX_BYTES
    assert arrs["extrinsic.npy"].shape == (2, 1, 3, 4)
    np.testing.assert_array_equal(arrs["extrinsic.npy"], torch.stack([r["extrinsic"] for r in results]).float().numpy())
    np.testing.assert_array_equal(arrs["cam_tokens.npy"], torch.stack([r["cam_tokens"] for r in results]).float().numpy())
    idx = torch.randint(0, big.numel(), (bench.DUMP_SAMPLE_ELEMS,), generator=torch.Generator().manual_seed(0)).sort().values
    np.testing.assert_array_equal(arrs["rgbs.npy"], big.reshape(-1)[idx].numpy())
    for n in names:
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes()


@pytest.mark.gpu
def test_bench_rccl_world1(tmp_path):
    """The RCCL process-group path of bench.py (init, ranks_seen all_gather_object, max-over-ranks
    all_reduce) at world 1 on the box's GPU, on a 2-view @518 step; --full for the extra workload,
    --dump-outputs for the last timed step's results."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(29500 + os.getpid() % 1000))
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "1", "--warmup", "1", "--views", "2",
                        "--full", "--no-cpu-baseline", "--extras", "n64", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 1 and line["backend"] == "nccl"
    assert line["value"] > 0
    assert line["steps"] == 1 and line["ms_per_step"] == pytest.approx(2 / line["value"] * 1e3)
    (x,) = line["extra_configs"]  # the 64-view extra workload rides inside the one line
    assert x["name"] == "n64" and "error" not in x and x["value"] > 0
    (seen,) = line["ranks_seen"]
    assert seen["rank"] == 0 and seen["device"].startswith("cuda") and "pci_bus" in seen
    ext = np.load(tmp_path / "extrinsic.npy")  # one [1, 3, 4] camera per query view
    assert ext.dtype == np.float32 and ext.shape == (2, 1, 3, 4) and np.isfinite(ext).all()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cam_tokens.npy", "extrinsic.npy", "intrinsic.npy",
                                                          "rgbs.npy"]
