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


def _wide(x: torch.Tensor) -> torch.Tensor:
    """The dtype a reference op computes in: fp32, and fp64 for an fp64
    input, so a module cast with .double() is an fp64 reference end to end
    (tests/block_cases.py) instead of an fp32 one stored in fp64."""
    return x if x.dtype == torch.float64 else x.float()


def rms_norm(x: torch.Tensor, weight: Optional[torch.Tensor], eps: float = 1e-6) -> torch.Tensor:
    """RMSNorm over the last dim (FLUX qk-norm and single-stream norms)."""
    dtype = x.dtype
    xf = _wide(x)
    rrms = torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)
    out = xf * rrms
    if weight is not None:
        out = out * _wide(weight)
    return out.to(dtype)


def layer_norm_mod(
    x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, eps: float = 1e-6
) -> torch.Tensor:
    """AdaLN-modulated LayerNorm: LN(x) * (1 + scale) + shift.

    x: [B, S, D]; scale/shift: [B, D] (broadcast over S) or [B, S, D].
    No learned affine — modulation plays that role (MMDiT convention).
    """
    dtype = x.dtype
    out = F.layer_norm(_wide(x), (x.shape[-1],), eps=eps)
    if scale.dim() == x.dim() - 1:
        scale = scale.unsqueeze(1)
        shift = shift.unsqueeze(1)
    out = out * (1.0 + _wide(scale)) + _wide(shift)
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
    out = F.group_norm(_wide(x), num_groups,
                       _wide(weight) if weight is not None else None,
                       _wide(bias) if bias is not None else None, eps)
    return F.silu(out).to(dtype)


def check_group_norm(x, num_groups, weight, bias, channel_add):
    """The refusals of the channels-last GroupNorm launcher, raised on every
    device (RuntimeError) so that CPU and GPU runs take the same arguments.
    The launcher's own limits (dense channels-last, 16-bit, C % 8 == 0) are
    not refusals of the op: such inputs run here."""
    def refuse_unless(ok, msg):
        if not ok:
            raise RuntimeError(f"group_norm: {msg}")

    refuse_unless(x.dim() == 4, f"x must be [B, C, H, W], got "
                                f"{list(x.shape)}")
    B, C = x.shape[:2]
    refuse_unless(int(num_groups) >= 1 and C % int(num_groups) == 0,
                  f"C % groups != 0 (C = {C}, groups = {num_groups})")
    for name, t, shape in (("weight", weight, (C,)), ("bias", bias, (C,)),
                           ("channel_add", channel_add, (B, C))):
        if t is None:
            continue
        refuse_unless(tuple(t.shape) == shape,
                      f"{name} must be {list(shape)}, got {list(t.shape)}")
        refuse_unless(t.dtype == x.dtype,
                      f"{name} dtype ({t.dtype}) must match x ({x.dtype})")
        refuse_unless(t.device == x.device,
                      f"{name} is on {t.device}, x on {x.device}")
    refuse_unless(channel_add is None or channel_add.is_contiguous(),
                  "channel_add must be contiguous")


def group_norm(
    x: torch.Tensor,
    num_groups: int,
    weight: Optional[torch.Tensor] = None,
    bias: Optional[torch.Tensor] = None,
    eps: float = 1e-6,
    *,
    silu: bool = False,
    channel_add: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """GroupNorm of x [B, C, H, W] with optional SiLU: GN(x + channel_add),
    the [B, C] addend broadcast over the pixels and added in fp32 before the
    statistics (the sum is not rounded to x's dtype). The result has x's
    dtype and memory format: channels-last in, channels-last out."""
    check_group_norm(x, num_groups, weight, bias, channel_add)
    dtype = x.dtype
    nhwc = (not x.is_contiguous()
            and x.is_contiguous(memory_format=torch.channels_last))
    xf = _wide(x)
    if channel_add is not None:
        xf = xf + _wide(channel_add)[:, :, None, None]
    # one summation order for both memory formats
    out = F.group_norm(xf.contiguous(), num_groups,
                       _wide(weight) if weight is not None else None,
                       _wide(bias) if bias is not None else None, eps)
    if silu:
        out = F.silu(out)
    out = out.to(dtype)
    return out.contiguous(memory_format=torch.channels_last) if nhwc else out


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
    xf = _wide(x).reshape(B, H, S, D // 2, 2)
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
    return_lse: bool = False,
):
    """Plain attention, [B, H, S, D] -> [B, H, S, D]. fp32 softmax.

    return_lse: also return fp32 lse [B, H, Sq], the log of the sum over the
    row's visible keys of exp(scale * q.k), and -inf on a row that sees no
    key: (out, lse). Partial results over disjoint key sets combine exactly
    through it (attention_merge).

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
        kf = torch.where(seen, _wide(k), torch.zeros((), device=k.device))
        vf = torch.where(seen, _wide(v), torch.zeros((), device=v.device))
        s = torch.matmul(_wide(q), kf.transpose(-1, -2)) * scale
        s = s.masked_fill(~vis, float("-inf"))
        p = torch.softmax(s, dim=-1)
        # a row with no visible key: softmax over all -inf is NaN -> zeros
        p = torch.where(vis.any(dim=3, keepdim=True), p,
                        torch.zeros((), device=p.device))
        out = torch.matmul(p, vf).to(dtype)
        return (out, torch.logsumexp(s, dim=-1)) if return_lse else out
    if key_mask is None:
        s = torch.matmul(_wide(q), _wide(k).transpose(-1, -2)) * scale
        p = torch.softmax(s, dim=-1)
        out = torch.matmul(p, _wide(v)).to(dtype)
        return (out, torch.logsumexp(s, dim=-1)) if return_lse else out
    m = as_bool_key_mask(key_mask).to(q.device)
    if m.shape != (q.shape[0], k.shape[2]):
        raise ValueError(f"key mask {tuple(m.shape)} does not match "
                         f"[B={q.shape[0]}, Sk={k.shape[2]}]")
    rows = m[:, None, :, None]                      # [B, 1, Sk, 1]
    kf = torch.where(rows, _wide(k), torch.zeros((), device=k.device))
    vf = torch.where(rows, _wide(v), torch.zeros((), device=v.device))
    s = torch.matmul(_wide(q), kf.transpose(-1, -2)) * scale
    s = s.masked_fill(~m[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    # all keys masked: softmax over all -inf is NaN; the contract is zeros
    p = torch.where(m.any(dim=1)[:, None, None, None], p,
                    torch.zeros((), device=p.device))
    out = torch.matmul(p, vf).to(dtype)
    # logsumexp of a row of -inf is -inf (of an empty row too)
    return (out, torch.logsumexp(s, dim=-1)) if return_lse else out


MERGE_MAX = 8       # partials per attention_merge: the GPUs of one node


def check_merge(outs, lses):
    """What attention_merge takes, on every device: 1 to MERGE_MAX partials
    (ValueError otherwise) of one shape, dtype and device, each with an fp32
    lse of its shape without the last dim on its device (RuntimeError
    otherwise, as from the native launcher)."""
    n = len(outs)
    if not 1 <= n <= MERGE_MAX:
        raise ValueError(f"attention_merge takes 1 to {MERGE_MAX} partials "
                         f"(one per GPU of a node), got {n}")
    if len(lses) != n:
        raise ValueError(f"attention_merge: {n} outs but {len(lses)} lses")
    o0 = outs[0]
    if o0.dim() < 1:
        raise RuntimeError("attention_merge: partials need a last dim D")
    for c, (o, l) in enumerate(zip(outs, lses)):
        if o.device != o0.device or l.device != o0.device:
            raise RuntimeError(
                f"attention_merge: partial {c} is on {o.device} (lse on "
                f"{l.device}), partial 0 on {o0.device}")
        if o.dtype != o0.dtype:
            raise RuntimeError(
                f"attention_merge: partial {c} dtype ({o.dtype}) must match "
                f"partial 0 ({o0.dtype})")
        if l.dtype != torch.float32:
            raise RuntimeError(
                f"attention_merge: lse {c} must be fp32, got {l.dtype}")
        if o.shape != o0.shape:
            raise RuntimeError(
                f"attention_merge: partial {c} has shape {list(o.shape)}, "
                f"partial 0 {list(o0.shape)}")
        if l.shape != o0.shape[:-1]:
            raise RuntimeError(
                f"attention_merge: lse {c} has shape {list(l.shape)}, its "
                f"partial needs {list(o0.shape[:-1])}")


def attention_merge(outs, lses, return_lse: bool = False):
    """N partial attention results [..., D] over disjoint key sets and their
    fp32 lse [...] -> the result over the union, in fp32 with one rounding:
    m = max_c lse_c, w_c = exp(lse_c - m), out = (sum_c w_c out_c) / sum_c
    w_c, lse = m + log sum_c w_c. A partial with lse_c = -inf is skipped
    (its out_c is don't-care, NaN included); all -inf gives out = +0 and
    lse = -inf. N = 1 returns the partial bit for bit."""
    check_merge(outs, lses)
    dtype = outs[0].dtype
    L = torch.stack(list(lses))                         # [N, ...]
    m = L.amax(0)
    dead = torch.isinf(m) & (m < 0)
    w = torch.exp(L - torch.where(dead, torch.zeros_like(m), m))
    live = ~(torch.isinf(L) & (L < 0))
    w = torch.where(live, w, torch.zeros_like(w))
    # the sum starts from -0.0, the exact identity of addition: a partial's
    # -0.0 survives N = 1
    acc = torch.full(outs[0].shape, -0.0, dtype=torch.float32,
                     device=outs[0].device)
    for c, o in enumerate(outs):
        acc = torch.where(live[c][..., None],
                          acc + w[c][..., None] * o.float(), acc)
    wsum = w.sum(0)
    out = torch.where(dead[..., None], torch.zeros_like(acc),
                      acc / wsum.clamp_min(1e-30)[..., None]).to(dtype)
    if not return_lse:
        return out
    return out, torch.where(dead, m, m + torch.log(wsum.clamp_min(1e-30)))


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
