"""Pure-PyTorch reference implementations of every custom op.

These are the numerics ground truth for the HIP kernels (tests compare the
gfx950 kernels against these run in fp32) and the CPU execution path for the
no-GPU test backend. They are NOT the GPU hot path — on HIP devices the
dispatch layer (ops/__init__.py) requires the native extension.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def rms_norm(x: torch.Tensor, weight: Optional[torch.Tensor], eps: float = 1e-6) -> torch.Tensor:
    """RMSNorm over the last dim (FLUX qk-norm and single-stream norms)."""
    dtype = x.dtype
    xf = x.float()
    rrms = torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)
    out = xf * rrms
    if weight is not None:
        out = out * weight.float()
    return out.to(dtype)


def layer_norm_mod(
    x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, eps: float = 1e-6
) -> torch.Tensor:
    """AdaLN-modulated LayerNorm: LN(x) * (1 + scale) + shift.

    x: [B, S, D]; scale/shift: [B, D] (broadcast over S) or [B, S, D].
    No learned affine — modulation plays that role (MMDiT convention).
    """
    dtype = x.dtype
    out = F.layer_norm(x.float(), (x.shape[-1],), eps=eps)
    if scale.dim() == x.dim() - 1:
        scale = scale.unsqueeze(1)
        shift = shift.unsqueeze(1)
    out = out * (1.0 + scale.float()) + shift.float()
    return out.to(dtype)


def gate_residual(residual: torch.Tensor, gate: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """residual + gate * x with gate [B, D] broadcast over sequence."""
    if gate.dim() == x.dim() - 1:
        gate = gate.unsqueeze(1)
    return residual + gate * x


def group_norm_silu(
    x: torch.Tensor,
    num_groups: int,
    weight: Optional[torch.Tensor],
    bias: Optional[torch.Tensor],
    eps: float = 1e-6,
) -> torch.Tensor:
    """GroupNorm + SiLU fused (UNet ResBlock prologue)."""
    dtype = x.dtype
    out = F.group_norm(x.float(), num_groups,
                       weight.float() if weight is not None else None,
                       bias.float() if bias is not None else None, eps)
    return F.silu(out).to(dtype)


def rope_freqs(
    positions: torch.Tensor, dim: int, theta: float = 10000.0
) -> torch.Tensor:
    """cos/sin table for rotary embedding.

    positions: [..., S] integer/float positions -> returns [..., S, dim/2, 2]
    stacked (cos, sin) in fp32. Axes composition (2D image RoPE) is done by
    the caller concatenating per-axis tables along the dim/2 axis.
    """
    half = dim // 2
    freqs = torch.arange(0, half, dtype=torch.float32, device=positions.device)
    inv = theta ** (-freqs / half)
    ang = positions.float().unsqueeze(-1) * inv  # [..., S, half]
    return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)


def rope_apply(x: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    """Apply rotary embedding.

    x: [B, H, S, D]; cs: [S, D/2, 2] or [B, S, D/2, 2] fp32 (cos,sin).
    Pairs are adjacent elements (x0,x1),(x2,x3)...
    """
    dtype = x.dtype
    B, H, S, D = x.shape
    xf = x.float().reshape(B, H, S, D // 2, 2)
    if cs.dim() == 3:
        cos = cs[None, None, :, :, 0]
        sin = cs[None, None, :, :, 1]
    else:
        cos = cs[:, None, :, :, 0]
        sin = cs[:, None, :, :, 1]
    x0, x1 = xf[..., 0], xf[..., 1]
    out = torch.stack([x0 * cos - x1 * sin, x0 * sin + x1 * cos], dim=-1)
    return out.reshape(B, H, S, D).to(dtype)


def as_bool_key_mask(mask: torch.Tensor) -> torch.Tensor:
    """[B, Sk] bool/integer key mask (nonzero = attend) -> bool.

    Floating masks are refused: a float tensor could be a 0/1 mask or a
    0/-inf additive bias, and guessing wrong silently inverts the mask.
    """
    if mask.dtype.is_floating_point or mask.dtype.is_complex:
        raise ValueError(
            f"key mask must be bool or integer (nonzero = attend), got "
            f"{mask.dtype}: additive float biases are not supported")
    if mask.dim() != 2:
        raise ValueError(f"key mask must be [B, Sk], got {tuple(mask.shape)}")
    return mask if mask.dtype == torch.bool else mask != 0


# Block-mask granularity: the attention kernel's geometry, 256 query rows by
# 64 keys (ops.ATTN_Q_BLOCK / ops.ATTN_KV_TILE).
Q_BLOCK = 256
KV_TILE = 64


def block_mask_shape(Sq: int, Sk: int) -> Tuple[int, int]:
    return (Sq + Q_BLOCK - 1) // Q_BLOCK, (Sk + KV_TILE - 1) // KV_TILE


def as_bool_block_mask(mask: torch.Tensor, Sq: int, Sk: int) -> torch.Tensor:
    """[ceil(Sq/256), ceil(Sk/64)] bool/integer block mask (nonzero = the
    query block attends the key tile) -> bool. Floating masks are refused
    for as_bool_key_mask's reason; another shape raises ValueError."""
    if mask.dtype.is_floating_point or mask.dtype.is_complex:
        raise ValueError(
            f"block mask must be bool or integer (nonzero = attend), got "
            f"{mask.dtype}: additive float biases are not supported")
    want = block_mask_shape(Sq, Sk)
    if tuple(mask.shape) != want:
        raise ValueError(
            f"block mask must be [ceil(Sq/{Q_BLOCK}), ceil(Sk/{KV_TILE})] = "
            f"{list(want)} for Sq={Sq}, Sk={Sk}, got {list(mask.shape)}")
    return mask if mask.dtype == torch.bool else mask != 0


def check_qkv(q, k, v, bshd: bool = False, split: Optional[int] = None):
    """k and v must have q's batch, head count and head dim, and one length
    between them; ``split`` lies inside (0, Sq). The native kernel indexes k
    and v with q's counts and would read past a smaller tensor, so nothing
    is broadcast, on any device, and the refusal comes before any mask is
    packed. Returns (Sq, Sk)."""
    if not (q.dim() == 4 and k.dim() == 4 and v.dim() == 4):
        raise ValueError(f"attention expects 4-D q/k/v, got {q.dim()}-D, "
                         f"{k.dim()}-D, {v.dim()}-D")
    s_ax, h_ax = (1, 2) if bshd else (2, 1)
    for name, ax in (("batch", 0), ("heads", h_ax), ("head dim", 3)):
        if not k.shape[ax] == v.shape[ax] == q.shape[ax]:
            raise ValueError(
                f"attention: k/v {name} must equal q's {name} "
                f"({q.shape[ax]}), got k {k.shape[ax]}, v {v.shape[ax]}")
    Sq, Sk = q.shape[s_ax], k.shape[s_ax]
    if v.shape[s_ax] != Sk:
        raise ValueError(f"attention: v must have k's length ({Sk} keys), "
                         f"got {v.shape[s_ax]}")
    if split is not None and not 0 < int(split) < Sq:
        raise ValueError(f"attention: split must lie inside (0, S = {Sq}), "
                         f"got {split}")
    return Sq, Sk


def attention(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float] = None,
    key_mask: Optional[torch.Tensor] = None,
    block_mask: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Plain attention, [B, H, S, D] -> [B, H, S, D]. fp32 softmax.

    key_mask: optional [B, Sk] bool/integer, nonzero = attend. Masked K/V
    rows are don't-care (zeroed before the matmuls, so NaN/Inf there never
    reaches the result), masked scores go to -inf, and a batch element with
    no live key gives zeros.

    block_mask: optional [ceil(Sq/256), ceil(Sk/64)] bool/integer, shared by
    batch and heads; nonzero = the 256-row query block attends the 64-key
    tile. Key j is visible to query row i of batch element b iff
    block_mask[i // 256][j // 64] and (no key mask or key_mask[b][j]). K/V
    rows at keys no query row of that batch element sees are don't-care
    (zeroed before the matmuls), and a query row with no visible key gives
    zeros.

    k and v have q's batch, head count and head dim (ValueError otherwise:
    nothing is broadcast, as on the native kernels). Sk = 0 gives zeros.
    """
    check_qkv(q, k, v)
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    dtype = q.dtype
    if block_mask is not None:
        Sq, Sk = q.shape[2], k.shape[2]
        bm = as_bool_block_mask(block_mask, Sq, Sk).to(q.device)
        vis = bm.repeat_interleave(Q_BLOCK, dim=0).repeat_interleave(
            KV_TILE, dim=1)[None, None, :Sq, :Sk]       # [1, 1, Sq, Sk]
        if key_mask is not None:
            m = as_bool_key_mask(key_mask).to(q.device)
            if m.shape != (q.shape[0], Sk):
                raise ValueError(f"key mask {tuple(m.shape)} does not match "
                                 f"[B={q.shape[0]}, Sk={Sk}]")
            vis = vis & m[:, None, None, :]             # [B, 1, Sq, Sk]
        seen = vis.any(dim=2)[..., None]                # [B|1, 1, Sk, 1]
        kf = torch.where(seen, k.float(), torch.zeros((), device=k.device))
        vf = torch.where(seen, v.float(), torch.zeros((), device=v.device))
        s = torch.matmul(q.float(), kf.transpose(-1, -2)) * scale
        s = s.masked_fill(~vis, float("-inf"))
        p = torch.softmax(s, dim=-1)
        # a row with no visible key: softmax over all -inf is NaN -> zeros
        p = torch.where(vis.any(dim=3, keepdim=True), p,
                        torch.zeros((), device=p.device))
        return torch.matmul(p, vf).to(dtype)
    if key_mask is None:
        s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
        p = torch.softmax(s, dim=-1)
        return torch.matmul(p, v.float()).to(dtype)
    m = as_bool_key_mask(key_mask).to(q.device)
    if m.shape != (q.shape[0], k.shape[2]):
        raise ValueError(f"key mask {tuple(m.shape)} does not match "
                         f"[B={q.shape[0]}, Sk={k.shape[2]}]")
    rows = m[:, None, :, None]                      # [B, 1, Sk, 1]
    kf = torch.where(rows, k.float(), torch.zeros((), device=k.device))
    vf = torch.where(rows, v.float(), torch.zeros((), device=v.device))
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * scale
    s = s.masked_fill(~m[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    # all keys masked: softmax over all -inf is NaN; the contract is zeros
    p = torch.where(m.any(dim=1)[:, None, None, None], p,
                    torch.zeros((), device=p.device))
    return torch.matmul(p, vf).to(dtype)


def timestep_embedding(
    t: torch.Tensor, dim: int, max_period: float = 10000.0, time_factor: float = 1000.0
) -> torch.Tensor:
    """Sinusoidal timestep embedding, fp32 in/out [B, dim]."""
    t = t.float() * time_factor
    half = dim // 2
    freqs = torch.exp(
        -math.log(max_period)
        * torch.arange(half, dtype=torch.float32, device=t.device)
        / half
    )
    args = t[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, emb.new_zeros(emb.shape[0], 1)], dim=-1)
    return emb
