"""GroupNorm+SiLU op timing: the NCHW op (ops.group_norm_silu) against the
channels-last op (ops.group_norm(..., silu=True)) on the same logical
tensors, alternating.

By default the shapes are read from a forward pre-hook on every GNSiLU and
SpatialTransformer of the full SDXL UNet at --batch / --px (one forward);
--shapes "B,C,H,W,G;..." gives them by hand. Each op is timed with device
events over --iters calls per round, rotating through enough input buffers
to exceed the 256 MiB last-level cache, and reported as ms per call and
effective GB/s for one read plus one write of the tensor.

    python scripts/bench_gn.py --batch 4 --px 1024 --rounds 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from comfyui_parallelanything_amd import ops  # noqa: E402
from comfyui_parallelanything_amd.models import sd_unet as U  # noqa: E402
from comfyui_parallelanything_amd.models.registry import (  # noqa: E402
    make_sdxl, sdxl_inputs)

ROOFLINE_GBS = 6300.0
CACHE_BYTES = 256 << 20


def model_shapes(batch: int, px: int, dtype) -> dict:
    """{(B, C, H, W, G): calls per forward} of the SDXL UNet's GroupNorms."""
    model = make_sdxl(dev="cuda", dtype=dtype)
    seen: dict = {}

    def hook(mod, args):
        x = args[0]
        G = mod.groups if isinstance(mod, U.GNSiLU) else mod.norm.num_groups
        key = tuple(x.shape) + (G,)
        seen[key] = seen.get(key, 0) + 1

    for mod in model.modules():
        if isinstance(mod, (U.GNSiLU, U.SpatialTransformer)):
            mod.register_forward_pre_hook(hook)
    x, t, c, kw = sdxl_inputs(batch, px=px, dev="cuda", dtype=dtype)
    with torch.no_grad():
        model(x, t, context=c, **kw)
    torch.cuda.synchronize()
    del model
    torch.cuda.empty_cache()
    return seen


def time_op(fn, bufs, iters: int) -> float:
    """ms per call."""
    for i in range(3):
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(bufs[i % len(bufs)])
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--px", type=int, default=1024)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--shapes", default=None, metavar="B,C,H,W,G;...")
    ap.add_argument("--json", default=None, help="write the rows here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_gn.py measures on the GPU; none found")
    assert ops.hip_available("group_norm_nhwc"), "native extension missing"
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]

    if args.shapes:
        shapes = {tuple(int(v) for v in s.split(",")): 1
                  for s in args.shapes.split(";")}
    else:
        shapes = model_shapes(args.batch, args.px, dtype)

    rows = []
    print(f"{'B,C,H,W,G':>22} {'calls':>5} {'round':>5} "
          f"{'nchw ms':>9} {'GB/s':>7} {'nhwc ms':>9} {'GB/s':>7} "
          f"{'nhwc/nchw':>9}")
    for shape, calls in sorted(shapes.items(),
                               key=lambda kv: (-kv[0][2], kv[0][1])):
        B, C, H, W, G = shape
        nbytes = 2 * B * C * H * W * 2          # one read plus one write
        # inputs of one layout total at least twice the cache (1 GiB of
        # device memory for the two layouts at the smallest shapes)
        nbuf = max(2, -(-2 * CACHE_BYTES // (nbytes // 2)))
        g = torch.Generator(device="cuda").manual_seed(C)
        nchw = [torch.randn(B, C, H, W, device="cuda", generator=g).to(dtype)
                for _ in range(nbuf)]
        nhwc = [t.contiguous(memory_format=torch.channels_last)
                for t in nchw]
        w = torch.randn(C, device="cuda", generator=g).to(dtype)
        b = torch.randn(C, device="cuda", generator=g).to(dtype)
        for r in range(args.rounds):
            t0 = time_op(lambda t: ops.group_norm_silu(t, G, w, b), nchw,
                         args.iters)
            t1 = time_op(lambda t: ops.group_norm(t, G, w, b, silu=True),
                         nhwc, args.iters)
            row = dict(shape=list(shape), calls=calls, round=r,
                       nchw_ms=t0, nhwc_ms=t1,
                       nchw_gbs=nbytes / t0 / 1e6, nhwc_gbs=nbytes / t1 / 1e6,
                       roofline_gbs=ROOFLINE_GBS)
            rows.append(row)
            print(f"{','.join(map(str, shape)):>22} {calls:>5} {r:>5} "
                  f"{t0:>9.4f} {row['nchw_gbs']:>7.0f} "
                  f"{t1:>9.4f} {row['nhwc_gbs']:>7.0f} {t1 / t0:>9.3f}",
                  flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
