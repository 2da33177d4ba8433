"""Child of test_gpu_attn_lse.test_two_rank_ring_and_wan, one process per GPU
under torch.distributed.run: the ring and sequence-parallel tiny WAN over
RCCL against the single-process result, compared on every rank at the
tolerance test_gpu_engine.py uses for its bf16 models. Without a GPU the
same script runs over gloo in fp32 (a check of the script itself)."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from comfyui_parallelanything_amd import ops  # noqa: E402
from comfyui_parallelanything_amd.models.registry import (  # noqa: E402
    make_wan, wan_inputs,
)
from comfyui_parallelanything_amd.parallel import (  # noqa: E402
    install_sequence_parallel, ring_attention_bshd,
    uninstall_sequence_parallel,
)
from comfyui_parallelanything_amd.parallel.dist import (  # noqa: E402
    COMM_STATS, barrier, init_distributed,
)

RTOL = ATOL = 2e-2


def main():
    info = init_distributed()
    assert info.world_size == 2
    dev = info.device
    gpu = dev.type == "cuda"
    assert info.backend == ("nccl" if gpu else "gloo")
    dtype = torch.bfloat16 if gpu else torch.float32
    g = torch.Generator(device="cpu").manual_seed(21)
    qkv = torch.randn(1, 600, 3, 4, 64, generator=g).to(dtype).to(dev)
    q, k, v = qkv.unbind(2)
    want = ops.attention_bshd(q, k, v)
    lo = 300 * info.rank
    before = COMM_STATS.sent_bytes
    out = ring_attention_bshd(q[:, lo:lo + 300], k[:, lo:lo + 300],
                              v[:, lo:lo + 300], None, [300, 300], info)
    torch.testing.assert_close(out, want[:, lo:lo + 300], rtol=RTOL, atol=ATOL)
    assert COMM_STATS.sent_bytes - before == 2 * 300 * 4 * 64 * (
        2 if gpu else 4)

    model = make_wan(dev=dev, dtype=dtype, tiny=True)
    x, t, c, kw = wan_inputs(1, dev=dev, dtype=dtype, tiny=True)
    ref = model(x, t, context=c, **kw)
    install_sequence_parallel(model, info)
    out = model(x, t, context=c, **kw)
    torch.testing.assert_close(out, ref, rtol=RTOL, atol=ATOL)
    assert uninstall_sequence_parallel(model)
    assert torch.equal(model(x, t, context=c, **kw), ref)
    if gpu:
        assert not ops._WARNED, ops._WARNED     # no reference-path fallback
        torch.cuda.synchronize()
    barrier(info)
    dist.destroy_process_group()
    print(f"rank {info.rank}: ok")


if __name__ == "__main__":
    main()
