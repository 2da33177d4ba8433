"""Sequence parallelism over gloo on the CPU: ring self-attention against the
gathered reference, and token-sharded WAN against the local forward."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from comfyui_parallelanything_amd.parallel.dist import COMM_STATS, DistInfo

RTOL, ATOL = 1e-5, 1e-6         # test_dist_pipeline.py's, same comparison
B, H, S, D = 2, 3, 37, 16
SIZES = {2: [37, 0], 3: [20, 0, 17]}    # uneven, one rank with no token


def _init(rank, world, tmpdir):
    dist.init_process_group(
        "gloo", init_method=f"file://{os.path.join(tmpdir, 'store')}",
        rank=rank, world_size=world,
    )
    return DistInfo(rank=rank, world_size=world, local_rank=rank,
                    device=torch.device("cpu"), backend="gloo")


def _ring_worker(rank, world, tmpdir, sizes):
    from comfyui_parallelanything_amd.ops import reference
    from comfyui_parallelanything_amd.parallel.sequence import (
        ring_attention_bshd,
    )

    info = _init(rank, world, tmpdir)
    g = torch.Generator().manual_seed(11)           # same data everywhere
    qkv = torch.randn(B, S, 3, H, D, generator=g)   # the fused GEMM's output
    q, k, v = qkv.unbind(2)
    want = reference.attention(*(t.permute(0, 2, 1, 3) for t in (q, k, v)),
                               0.3).permute(0, 2, 1, 3)
    lo = sum(sizes[:rank])
    hi = lo + sizes[rank]
    before = COMM_STATS.sent_bytes, COMM_STATS.recv_bytes
    out = ring_attention_bshd(q[:, lo:hi], k[:, lo:hi], v[:, lo:hi], 0.3,
                              sizes, info)
    assert out.shape == (B, sizes[rank], H, D)
    torch.testing.assert_close(out, want[:, lo:hi], rtol=RTOL, atol=ATOL)
    # this rank forwards the shards that started on rank, rank - 1, ...,
    # rank - (world - 2), and receives those of rank - 1, ..., rank - (world
    # - 1): K and V of 2 * B * H * D fp32 values per token
    per_token = 2 * B * H * D * 4
    sent = sum(sizes[(rank - i) % world] for i in range(world - 1))
    recv = sum(sizes[(rank - i - 1) % world] for i in range(world - 1))
    assert COMM_STATS.sent_bytes - before[0] == per_token * sent
    assert COMM_STATS.recv_bytes - before[1] == per_token * recv
    with pytest.raises(ValueError, match="sizes"):
        ring_attention_bshd(q, k, v, 0.3, [S + 1] * world, info)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ring_attention_uneven_shards(world, tmp_path):
    mp.spawn(_ring_worker, args=(world, str(tmp_path), SIZES[world]),
             nprocs=world, join=True)


def test_ring_even_bytes_formula(tmp_path):
    """Equal shards: every rank sends (N - 1) * 2 * B * H * D * elem * S/N."""
    mp.spawn(_even_worker, args=(2, str(tmp_path)), nprocs=2, join=True)


def _even_worker(rank, world, tmpdir):
    from comfyui_parallelanything_amd.parallel.sequence import (
        ring_attention_bshd, shard_sizes,
    )

    info = _init(rank, world, tmpdir)
    sizes = shard_sizes(36, world)
    assert sizes == [18, 18] and shard_sizes(37, 3) == [13, 12, 12]
    q = torch.randn(B, 18, H, D)
    before = COMM_STATS.sent_bytes
    ring_attention_bshd(q, q, q, None, sizes, info)
    assert COMM_STATS.sent_bytes - before == (world - 1) * 2 * B * H * D * 4 * 18
    dist.destroy_process_group()


def _wan_worker(rank, world, tmpdir, i2v, masked):
    from comfyui_parallelanything_amd.models import registry
    from comfyui_parallelanything_amd.parallel import (
        install_sequence_parallel, uninstall_sequence_parallel,
    )

    info = _init(rank, world, tmpdir)
    make, inputs = ((registry.make_wan_i2v, registry.wan_i2v_inputs) if i2v
                    else (registry.make_wan, registry.wan_inputs))
    model = make(tiny=True, dtype=torch.float32)    # same seed everywhere
    x, t, c, kw = inputs(1, tiny=True, dtype=torch.float32,
                         text_len=5 if masked else None)
    assert ("attention_mask" in kw) == masked
    ref = model(x, t, context=c, **kw)
    install_sequence_parallel(model, info)
    if rank != 0:
        # rank 0's inputs are the ones that count
        x, c = torch.zeros_like(x), torch.ones_like(c)
    keep = x.clone()
    out = model(x, t, context=c, **kw)
    torch.testing.assert_close(out, ref, rtol=RTOL, atol=ATOL)
    assert torch.equal(x, keep), "the caller's tensor was written"
    assert uninstall_sequence_parallel(model)
    if rank == 0:
        assert torch.equal(model(x, t, context=c, **kw), ref)
    dist.destroy_process_group()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masked"])
@pytest.mark.parametrize("i2v", [False, True], ids=["t2v", "i2v"])
@pytest.mark.parametrize("world", [2, 3])
def test_wan_sequence_parallel(world, i2v, masked, tmp_path):
    mp.spawn(_wan_worker, args=(world, str(tmp_path), i2v, masked),
             nprocs=world, join=True)


def test_frame_window_is_refused():
    from comfyui_parallelanything_amd.models.registry import (
        make_wan, wan_inputs,
    )
    from comfyui_parallelanything_amd.parallel import (
        install_sequence_parallel, uninstall_sequence_parallel,
    )

    info = DistInfo(0, 1, 0, torch.device("cpu"), "gloo")
    model = make_wan(tiny=True, dtype=torch.float32)
    x, t, c, kw = wan_inputs(1, tiny=True, dtype=torch.float32)
    ref = model(x, t, context=c, **kw)
    model.cfg.self_attn_frame_window = 1
    with pytest.raises(ValueError, match="frame_window"):
        install_sequence_parallel(model, info)
    model.cfg.self_attn_frame_window = None
    install_sequence_parallel(model, info)      # one rank: ring of one
    torch.testing.assert_close(model(x, t, context=c, **kw), ref,
                               rtol=RTOL, atol=ATOL)
    model.cfg.self_attn_frame_window = 1
    with pytest.raises(ValueError, match="frame_window"):
        model(x, t, context=c, **kw)
    model.cfg.self_attn_frame_window = None
    assert uninstall_sequence_parallel(model)
    assert not uninstall_sequence_parallel(model)
    assert torch.equal(model(x, t, context=c, **kw), ref)
    with pytest.raises(TypeError, match="WanDiT"):
        install_sequence_parallel(torch.nn.Linear(2, 2), info)
