"""End-to-end bench.py step-loop tests at world 4 and 8 over gloo.

VERDICT round-1 item 1: before the first real 8-GPU run, the EXACT loop the
driver benches (scatterv -> forward -> gatherv -> all_max, weighted sizes,
template paths, zero-size ranks) must pass multi-process on CPU. These
tests call ``bench.main`` itself — not a reimplementation — so every
collective call site, the routing of --weights, and the result contract are
exercised as a unit. The gloo backend runs the identical torch.distributed
call pattern RCCL runs on MI355X.

Every bench.main call here runs in a spawned worker that reports no HIP
device, so the loop takes its CPU/gloo path on a GPU machine too (N ranks
cannot share one GPU under RCCL, and the checksums compare CPU math).
"""
import json
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE_ARGS = [
    "--model", "sd15", "--tiny", "--steps", "2", "--warmup", "1",
    "--px", "64",
]


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bench_worker(rank, world, port, json_path, extra_argv):
    # CPU/gloo path regardless of the host: bench.py and init_distributed
    # pick device, dtype and backend from this probe alone
    torch.cuda.is_available = lambda: False
    os.environ["RANK"] = str(rank)
    os.environ["LOCAL_RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.manual_seed(0)  # identical random-init weights on every rank
    torch.set_num_threads(1)
    sys.path.insert(0, REPO_ROOT)
    import bench

    res = bench.main(list(extra_argv))
    if rank == 0:
        with open(json_path, "w") as f:
            json.dump(res, f)
    import torch.distributed as dist

    if dist.is_initialized():
        dist.destroy_process_group()


def _run_world(world, tmp_path, extra_argv, base=None):
    # argv travels as a spawn argument: workers re-import this module, so
    # nothing patched in the parent would reach them
    extra_argv = list(BASE_ARGS if base is None else base) + list(extra_argv)
    port = _free_port()
    out = str(tmp_path / f"bench_w{world}.json")
    mp.spawn(
        _bench_worker,
        args=(world, port, out, extra_argv),
        nprocs=world,
        join=True,
    )
    with open(out) as f:
        return json.load(f)


def _single_proc_reference(extra_argv, tmp_path, base=None):
    """bench.main at world 1, same seed -> checksum ground truth."""
    return _run_world(1, tmp_path, extra_argv, base)


@pytest.mark.parametrize("world", [4, 8])
def test_bench_step_loop_matches_single_process(world, tmp_path):
    """N-rank scatter/forward/gather must produce the same final latent as
    the single-process run (CPU math is bitwise chunk-stable)."""
    extra = ["--batch", "8"]
    ref = _single_proc_reference(extra, tmp_path)
    res = _run_world(world, tmp_path, extra)
    assert res["n_gpus"] == world
    assert res["ms_per_step"] > 0
    assert res["config"]["parallelism"] == f"dp{world}"
    assert res["x_checksum"] == pytest.approx(ref["x_checksum"], rel=1e-5)


def test_bench_weighted_split_world4(tmp_path):
    """The Z-Image-style weighted split path (--weights) at world 4."""
    extra = ["--batch", "8", "--weights", "40,30,20,10"]
    ref = _single_proc_reference(["--batch", "8"], tmp_path)
    res = _run_world(4, tmp_path, extra)
    assert "weighted" in res["config"]["parallelism"]
    assert res["x_checksum"] == pytest.approx(ref["x_checksum"], rel=1e-5)


def test_bench_zero_size_ranks_world4(tmp_path):
    """batch < world leaves some ranks with zero-size chunks — the loop
    (incl. the source rank holding a 0-row slice) must not deadlock."""
    extra = ["--batch", "2"]
    ref = _single_proc_reference(extra, tmp_path)
    res = _run_world(4, tmp_path, extra)
    assert res["x_checksum"] == pytest.approx(ref["x_checksum"], rel=1e-5)


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last step's eps/x as float32 .npy, equal
    from run to run with equal arguments; --full is accepted."""
    import numpy as np

    extra = ["--batch", "2"]
    res = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = _single_proc_reference(
            extra + ["--dump-outputs", str(d), "--full"], tmp_path)
        assert r["steps"] == 2 and r["ms_per_step"] > 0
        assert sorted(p.name for p in d.iterdir()) == ["eps.npy", "x.npy"]
        res.append({p.stem: np.load(p) for p in d.iterdir()})
    for k, a in res[0].items():
        assert a.dtype == np.float32 and a.shape[0] == 2
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, res[1][k])
    assert float(np.abs(res[0]["x"]).mean()) == pytest.approx(
        r["x_checksum"], rel=1e-5)


def test_bench_dump_outputs_sampled_when_large(tmp_path, monkeypatch):
    """Arrays past the size budget are cut to a fixed seeded sample."""
    import numpy as np

    sys.path.insert(0, REPO_ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 8192)
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    small = torch.ones(3, 5, dtype=torch.bfloat16)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), {"big": big, "small": small})
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.dtype == np.float32 and a.ndim == 1 and a.nbytes <= 8192 - 4096
    assert np.all(np.diff(a) > 0)  # sorted indices into an arange: a subset
    np.testing.assert_array_equal(a, np.load(tmp_path / "b" / "big.npy"))
    assert np.load(tmp_path / "a" / "small.npy").shape == (3, 5)
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert total <= 2 * 8192


def test_bench_wan_i2v_world2(tmp_path):
    """wan_i2v through the process-group loop at world 2: 5-D latents and
    the batch-shaped image_cond kwarg ride scatterv/gatherv."""
    extra = ["--batch", "4"]
    base = [a for a in BASE_ARGS]
    base[base.index("sd15")] = "wan_i2v"
    # remove --px (wan path takes no px inputs)
    i = base.index("--px")
    del base[i:i + 2]
    ref = _single_proc_reference(extra, tmp_path, base)
    res = _run_world(2, tmp_path, extra, base)
    assert "WAN2.2-class I2V" in res["config"]["model"]
    assert res["n_gpus"] == 2
    assert res["x_checksum"] == pytest.approx(ref["x_checksum"], rel=1e-5)
