#!/usr/bin/env python3
"""Attention / op microbench on MI355X (run under gpurun).

Reports TF/s for the fused attention kernel at FLUX/SDXL/WAN shapes and
times the per-layer fused ops; also a hipBLASLt bf16 GEMM reference to show
the roofline context. Random data (guide §5.4 rule 25).

--dtype {bf16,fp16} picks the element type of the attention and fused-op
sections (default bf16); the hipBLASLt reference stays bf16. --attn-only
stops after the attention section (for dtype A/B runs).

--key-mask {none,full,lens} runs the attention section with a key-padding
mask, packed once outside the timed loop as the models do per forward:
full = all keys live (the masked kernel's overhead against none), lens = the
first --live-keys keys of every batch element live (tile skipping). TF/s
always counts the dense Sq x Sk problem, so it is comparable across modes.

--frames F runs one shape instead of the table: WAN 720p self-attention, B1
H40 D128 over S = F x 3600 tokens (F = 21 gives 75 600). --block-mask
{none,full,frame:W} adds a block mask, packed once outside the timed loop
(with the key mask, if any): full = every block live (the block-list
kernel's overhead against --key-mask full), frame:W = the frame window of
ops.frame_window_block_mask (needs --frames). The mask density — live
256x64 blocks over all blocks — is printed beside each time.

--shape B,H,Sq,Sk,D runs that one shape instead of the table. --lse times
ops.attention_lse (the LSE instantiations: one more store per row) in place
of ops.attention; it takes no block mask.

--ring-chunks N prices sequence parallelism's chunking on ONE GPU, with no
interconnect in the picture: at --shape (default B1 H40 Sq9450 Sk75600 D128,
one of eight ranks' queries against every key of WAN 720p x 21 frames) it
times the dense call, then N attention_lse calls over N contiguous key
chunks plus the attention_merge, then the merge alone in GB/s."""
import argparse
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from comfyui_parallelanything_amd import ops  # noqa: E402


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def attn_flops(B, H, S, D, Sk=None):
    # QK^T + PV, 2 FLOP per MAC
    return 4.0 * B * H * S * (S if Sk is None else Sk) * D


def ring_chunks(n, shape, dtype, dev):
    """Dense attention against n chunk calls + merge, and the merge alone."""
    B, H, S, Sk, D = shape
    print(f"== ring chunks: B{B} H{H} Sq{S} Sk{Sk} D{D}, {n} chunks "
          f"({dtype}, random data) ==")
    q = torch.randn(B, H, S, D, device=dev, dtype=dtype)
    k = torch.randn(B, H, Sk, D, device=dev, dtype=dtype)
    v = torch.randn_like(k)
    # each chunk a buffer of its own, as it arrives from the ring
    cuts = [Sk // n + (1 if c < Sk % n else 0) for c in range(n)]
    ks = [t.contiguous() for t in k.split(cuts, dim=2)]
    vs = [t.contiguous() for t in v.split(cuts, dim=2)]

    def chunked():
        parts = [ops.attention_lse(q, kc, vc) for kc, vc in zip(ks, vs)]
        return ops.attention_merge([p[0] for p in parts],
                                   [p[1] for p in parts])

    parts = [ops.attention_lse(q, kc, vc) for kc, vc in zip(ks, vs)]
    outs, lses = [p[0] for p in parts], [p[1] for p in parts]
    dense = timeit(lambda: ops.attention(q, k, v), iters=10)
    split = timeit(chunked, iters=10)
    merge = timeit(lambda: ops.attention_merge(outs, lses), iters=20)
    nbytes = (n + 1) * outs[0].numel() * 2 + n * lses[0].numel() * 4
    tf = attn_flops(B, H, S, D, Sk) / 1e12
    print(f"  dense:            {dense*1e3:8.3f} ms  {tf/dense:7.1f} TF/s")
    print(f"  {n} chunks + merge: {split*1e3:8.3f} ms  {tf/split:7.1f} TF/s  "
          f"({split/dense:.4f} of dense)")
    print(f"  merge alone:      {merge*1e3:8.3f} ms  "
          f"{nbytes/merge/1e9:7.0f} GB/s ({nbytes/1e6:.1f} MB)")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--key-mask", choices=("none", "full", "lens"),
                    default="none")
    ap.add_argument("--live-keys", type=int, default=64,
                    help="live keys per batch element for --key-mask lens")
    ap.add_argument("--block-mask", default="none", metavar="none|full|frame:W")
    ap.add_argument("--frames", type=int, default=0,
                    help="run the WAN 720p shape with this many latent "
                         "frames (3600 tokens each) instead of the table")
    ap.add_argument("--shape", default="", metavar="B,H,Sq,Sk,D")
    ap.add_argument("--lse", action="store_true",
                    help="time ops.attention_lse instead of ops.attention")
    ap.add_argument("--ring-chunks", type=int, default=0, metavar="N")
    args = ap.parse_args()
    shape = None
    if args.shape:
        shape = tuple(int(x) for x in args.shape.split(","))
        if len(shape) != 5:
            ap.error("--shape takes B,H,Sq,Sk,D")
    if args.lse and args.block_mask != "none":
        ap.error("--lse takes no block mask")
    window = None
    if args.block_mask.startswith("frame:"):
        window = int(args.block_mask.split(":", 1)[1])
        if args.frames <= 0:
            ap.error("--block-mask frame:W needs --frames")
    elif args.block_mask not in ("none", "full"):
        ap.error("--block-mask takes none, full or frame:W")
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    assert torch.cuda.is_available()
    dev = "cuda"
    if args.ring_chunks:
        ring_chunks(args.ring_chunks, shape or (1, 40, 9450, 75600, 128),
                    dtype, dev)
        return
    attn = ops.attention_lse if args.lse else ops.attention
    print(f"== attention{' + lse' if args.lse else ''} ({args.dtype}, random data, "
          f"key mask: {args.key_mask}, block mask: {args.block_mask}) ==")
    tokens_per_frame = 3600  # 720p: (720/16) x (1280/16) latent patches
    video = {f"wan720p_f{args.frames}": (
        1, 40, args.frames * tokens_per_frame,
        args.frames * tokens_per_frame, 128)}
    if shape is not None:
        video = {"shape": shape}
    for name, (B, H, S, Sk, D) in (video if args.frames > 0 or shape else {
        "flux_b8": (8, 24, 4608, 4608, 128),
        "flux_b1": (1, 24, 4608, 4608, 128),
        "sdxl_mid": (4, 20, 1024, 1024, 64),
        "square_2k": (16, 16, 2048, 2048, 128),
        "zimage_b21": (21, 28, 4352, 4352, 128),  # joint 256 txt + 4096 img
        "cross_512": (21, 28, 4096, 512, 128),    # padded text context
    }).items():
        q = torch.randn(B, H, S, D, device=dev, dtype=dtype)
        k = torch.randn(B, H, Sk, D, device=dev, dtype=dtype)
        v = torch.randn_like(k)
        km = None
        if args.key_mask != "none":
            live = Sk if args.key_mask == "full" else min(args.live_keys, Sk)
            km = ops.pack_key_mask(
                (torch.arange(Sk, device=dev) < live).expand(B, Sk))
        mk = {"key_mask": km}
        note = ""
        if args.block_mask != "none":
            nq, nk = ops.reference.block_mask_shape(S, Sk)
            block = (torch.ones(nq, nk, dtype=torch.bool, device=dev)
                     if window is None else ops.frame_window_block_mask(
                         args.frames, tokens_per_frame, window, device=dev))
            mk = {"block_mask": ops.pack_block_mask(block, B, S, Sk, km)}
            note = f"  density {block.float().mean().item():.4f}"
        dt = timeit(lambda: attn(q, k, v, **mk), iters=10)
        tf = attn_flops(B, H, S, D, Sk) / dt / 1e12
        print(f"  {name:10s} B{B} H{H} S{S} Sk{Sk} D{D}: {dt*1e3:8.2f} ms  "
              f"{tf:7.1f} TF/s{note}")
    if args.attn_only:
        return

    print("== hipBLASLt bf16 GEMM reference ==")
    for n in (4096, 8192):
        a = torch.randn(n, n, device=dev, dtype=torch.bfloat16)
        b = torch.randn(n, n, device=dev, dtype=torch.bfloat16)
        dt = timeit(lambda: a @ b, iters=10)
        print(f"  {n}^3: {dt*1e3:8.2f} ms  {2*n**3/dt/1e12:7.1f} TF/s")
    # FLUX linear shapes (M = batch*seq)
    for (m, k_, n) in [(36864, 3072, 3072), (36864, 3072, 12288),
                       (36864, 15360, 3072), (36864, 3072, 21504)]:
        a = torch.randn(m, k_, device=dev, dtype=torch.bfloat16)
        w = torch.randn(n, k_, device=dev, dtype=torch.bfloat16)
        dt = timeit(lambda: torch.nn.functional.linear(a, w), iters=10)
        print(f"  linear {m}x{k_}x{n}: {dt*1e3:8.2f} ms  {2*m*k_*n/dt/1e12:7.1f} TF/s")

    print(f"== fused elementwise ops ({args.dtype}, FLUX shapes, batch 8) ==")
    B, S, Dm = 8, 4608, 3072
    x = torch.randn(B, S, Dm, device=dev, dtype=dtype)
    sc = torch.randn(B, Dm, device=dev, dtype=dtype)
    sh = torch.randn_like(sc)
    dt = timeit(lambda: ops.layer_norm_mod(x, sc, sh))
    gbs = 2 * x.numel() * 2 / dt / 1e9
    print(f"  layer_norm_mod: {dt*1e3:7.3f} ms  {gbs:7.0f} GB/s")
    dt = timeit(lambda: ops.gate_residual(x, sc, x))
    print(f"  gate_residual:  {dt*1e3:7.3f} ms  {3*x.numel()*2/dt/1e9:7.0f} GB/s")
    qh = torch.randn(B, 24, S, 128, device=dev, dtype=dtype)
    w = torch.randn(128, device=dev, dtype=dtype)
    dt = timeit(lambda: ops.rms_norm(qh, w))
    print(f"  rms_norm qk:    {dt*1e3:7.3f} ms  {2*qh.numel()*2/dt/1e9:7.0f} GB/s")
    from comfyui_parallelanything_amd.ops import reference as R
    cs = R.rope_freqs(torch.arange(S, device=dev), 128)
    dt = timeit(lambda: ops.rope_apply(qh, cs))
    print(f"  rope_apply:     {dt*1e3:7.3f} ms  {2*qh.numel()*2/dt/1e9:7.0f} GB/s")


if __name__ == "__main__":
    main()
