"""UNet token op timing: the eager torch composition a TransformerBlock runs
by default against ops.layer_norm / ops.geglu on the same tensors,
alternating.

Shapes are the SDXL 1024^2 batch-4 token shapes, rows x width of the input:
C for the LayerNorms, 2N = 8 C for the GEGLU projection; --shapes
"op,rows,width;..." gives others.
Each side is timed with device events over --iters calls per round,
rotating through enough input buffers to exceed the 256 MiB last-level
cache, and reported as ms per call and effective GB/s for the bytes one
pass has to move, against the ~6300 GB/s roofline.

    python scripts/bench_token_ops.py --rounds 3

--grouped times the grouped modulation kernels instead (docs/KERNELS.md,
"Grouped modulation"): ops.layer_norm_mod and ops.gate_residual on x [1, S,
D] with [1, G, D] modulation, bf16, three kinds of run alternating per round:
(a) the composed reference path on the device with the modulation expanded
to [1, S, D] (expanded once, outside the timing), which was the only route
for such a call before the kernels; (b) the [B, D] kernels on the same x,
which move the same bytes; (c) the grouped kernels.

    python scripts/bench_token_ops.py --grouped --rounds 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from comfyui_parallelanything_amd import ops  # noqa: E402

ROOFLINE_GBS = 6300.0
CACHE_BYTES = 256 << 20
SHAPES = "ln,16384,640;ln,4096,1280;ln_add,16384,640;ln_add,4096,1280;" \
         "geglu,16384,5120;geglu,4096,10240"


def one_pass_bytes(op: str, rows: int, width: int) -> int:
    """What one pass has to move: ln reads x and writes y; ln_add reads x
    and delta and writes the sum and y; geglu reads width = 2N and writes
    N."""
    return {"ln": 4, "ln_add": 8, "geglu": 3}[op] * rows * width


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


def sides(op: str, width: int, dtype, g):
    """(eager, native) callables of one input buffer."""
    if op == "geglu":
        def eager(y):
            a, b = y.chunk(2, dim=-1)
            return a * F.gelu(b)
        return eager, ops.geglu
    w = torch.randn(width, device="cuda", generator=g).to(dtype)
    b = torch.randn(width, device="cuda", generator=g).to(dtype)
    if op == "ln":
        return (lambda x: F.layer_norm(x, (width,), w, b, 1e-5),
                lambda x: ops.layer_norm(x, w, b))

    def eager(xd):
        s = xd[0] + xd[1]
        return s, F.layer_norm(s, (width,), w, b, 1e-5)
    return eager, lambda xd: ops.layer_norm(xd[1], w, b, residual=xd[0])


GROUPED_SHAPES = ((75600, 21, 5120), (75600, 21, 3072))    # WAN 14B, 5B


def grouped(args):
    """(a) reference, (b) [B, D] kernels, (c) grouped kernels, alternating."""
    from comfyui_parallelanything_amd.ops import reference

    dtype = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    rows_out = []
    print(f"{'op S G D':>28} {'round':>5} {'(a) ms':>9} {'(b) ms':>9} "
          f"{'(c) ms':>9} {'(b) GB/s':>9} {'(c) GB/s':>9}")
    for S, G, D in GROUPED_SHAPES:
        def new(*shape):
            return torch.randn(*shape, device="cuda", generator=g).to(dtype)
        # x alone exceeds the last-level cache; two buffers alternate
        bufs = [(new(1, S, D), new(1, S, D)) for _ in range(2)]
        mod = new(1, G, 6, D).unbind(-2)        # the caller's strided views
        wide = [m.repeat_interleave(S // G, dim=1) for m in mod[:3]]
        flat = [m[:, 0] for m in mod[:3]]
        sides = {
            "layer_norm_mod": (
                lambda b: reference.layer_norm_mod(b[0], wide[0], wide[1]),
                lambda b: ops.layer_norm_mod(b[0], flat[0], flat[1]),
                lambda b: ops.layer_norm_mod(b[0], mod[0], mod[1]), 4),
            "gate_residual": (
                lambda b: reference.gate_residual(b[1], wide[2], b[0]),
                lambda b: ops.gate_residual(b[1], flat[2], b[0]),
                lambda b: ops.gate_residual(b[1], mod[2], b[0]), 6),
        }
        for op, (ref_fn, flat_fn, grp_fn, passes) in sides.items():
            nbytes = passes * S * D
            for r in range(args.rounds):
                ta = time_op(ref_fn, bufs, max(args.iters // 10, 3))
                tb = time_op(flat_fn, bufs, args.iters)
                tc = time_op(grp_fn, bufs, args.iters)
                row = dict(op=op, S=S, G=G, D=D, round=r, reference_ms=ta,
                           flat_ms=tb, grouped_ms=tc,
                           flat_gbs=nbytes / tb / 1e6,
                           grouped_gbs=nbytes / tc / 1e6)
                rows_out.append(row)
                print(f"{op + f' {S} {G} {D}':>28} {r:>5} {ta:>9.4f} "
                      f"{tb:>9.4f} {tc:>9.4f} {row['flat_gbs']:>9.0f} "
                      f"{row['grouped_gbs']:>9.0f}", flush=True)
        del bufs, mod, wide, flat, sides
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows_out, f, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--shapes", default=SHAPES, metavar="op,rows,width;...")
    ap.add_argument("--json", default=None, help="write the rows here")
    ap.add_argument("--grouped", action="store_true",
                    help="time the grouped modulation kernels instead")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_ops.py measures on the GPU; none found")
    if args.grouped:
        assert ops.hip_available("layer_norm_mod_grouped"), \
            "native extension missing"
        return grouped(args)
    assert ops.hip_available("layer_norm_affine"), "native extension missing"
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]

    rows_out = []
    print(f"{'op,rows,width':>22} {'round':>5} {'eager ms':>9} {'GB/s':>7} "
          f"{'op ms':>9} {'GB/s':>7} {'op/eager':>9}")
    for spec in args.shapes.split(";"):
        op, rows, width = spec.split(",")
        rows, width = int(rows), int(width)
        nbytes = one_pass_bytes(op, rows, width)
        in_elems = rows * width * (2 if op == "ln_add" else 1)
        nbuf = max(2, -(-2 * CACHE_BYTES // (in_elems * 2)))
        g = torch.Generator(device="cuda").manual_seed(width)

        def new(n_cols):
            return torch.randn(rows, n_cols, device="cuda",
                               generator=g).to(dtype)
        if op != "ln_add":
            bufs = [new(width) for _ in range(nbuf)]
        else:
            bufs = [(new(width), new(width)) for _ in range(nbuf)]
        eager, native = sides(op, width, dtype, g)
        for r in range(args.rounds):
            t0 = time_op(eager, bufs, args.iters)
            t1 = time_op(native, bufs, args.iters)
            row = dict(op=op, rows=rows, width=width, round=r, eager_ms=t0,
                       op_ms=t1, eager_gbs=nbytes / t0 / 1e6,
                       op_gbs=nbytes / t1 / 1e6, roofline_gbs=ROOFLINE_GBS)
            rows_out.append(row)
            print(f"{spec:>22} {r:>5} {t0:>9.4f} {row['eager_gbs']:>7.0f} "
                  f"{t1:>9.4f} {row['op_gbs']:>7.0f} {t1 / t0:>9.3f}",
                  flush=True)
        del bufs
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
