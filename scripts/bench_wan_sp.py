#!/usr/bin/env python3
"""Sequence-parallel WAN2.2 14B step time, one process per GPU.

    python -m torch.distributed.run --standalone --nproc_per_node N \\
        scripts/bench_wan_sp.py [--depth 4] [--frames 21] [--steps 5]

Batch 1, 720p (90 x 160 latent) x --frames latent frames, bf16, random
weights and data. Every rank holds the full weights and its shard of the
tokens (parallel.sequence.install_sequence_parallel); with N = 1 (also
without torch.distributed.run) the same path runs as a ring of one.
--depth builds that many of the 40 blocks (they all cost the same) and the
result line says which. Reports, as the maximum over ranks: ms per forward,
ms of ring transfer the attention did not hide (the compute stream's waits
on the K/V receives) and its share of the step, and the bytes each rank
sent per step. One JSON line on rank 0."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from comfyui_parallelanything_amd.models.registry import wan_inputs  # noqa: E402
from comfyui_parallelanything_amd.models.wan import WanConfig, WanDiT  # noqa: E402
from comfyui_parallelanything_amd.parallel import (  # noqa: E402
    install_sequence_parallel, sequence,
)
from comfyui_parallelanything_amd.parallel.dist import (  # noqa: E402
    COMM_STATS, all_max, barrier, init_distributed,
)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--depth", type=int, default=40)
    ap.add_argument("--frames", type=int, default=21)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--local", action="store_true",
                    help="nothing installed: the plain forward (N = 1 only)")
    args = ap.parse_args()
    info = init_distributed()
    assert info.device.type == "cuda", "needs HIP devices"
    cfg = WanConfig.wan22_a14b()
    cfg.depth = args.depth
    torch.manual_seed(0)
    with torch.device(info.device):
        model = WanDiT(cfg).to(dtype=torch.bfloat16).eval()
    x, t, ctx, kw = wan_inputs(1, frames=args.frames, dev=info.device)
    if not args.local:
        install_sequence_parallel(model, info)
    for _ in range(args.warmup):
        model(x, t, context=ctx, **kw)
    torch.cuda.synchronize()
    barrier(info)
    sequence.EXPOSED_WAIT_EVENTS = []
    sent0 = COMM_STATS.sent_bytes
    t0 = time.perf_counter()
    for _ in range(args.steps):
        model(x, t, context=ctx, **kw)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / args.steps * 1e3
    exposed_ms = sum(a.elapsed_time(b)
                     for a, b in sequence.EXPOSED_WAIT_EVENTS) / args.steps
    sequence.EXPOSED_WAIT_EVENTS = None
    step_ms = all_max(step_ms, info)
    exposed_ms = all_max(exposed_ms, info)
    if info.is_lead:
        print(json.dumps({
            "model": "wan22_a14b", "depth": args.depth, "frames": args.frames,
            "tokens": args.frames * 3600, "ranks": info.world_size,
            "sequence_parallel": not args.local,
            "ms_per_step": round(step_ms, 2),
            "ring_exposed_ms": round(exposed_ms, 2),
            "ring_exposed_share": round(exposed_ms / step_ms, 4),
            "sent_mb_per_rank_step": round(
                (COMM_STATS.sent_bytes - sent0) / args.steps / 1e6, 1),
        }))
    barrier(info)
    if info.world_size > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
