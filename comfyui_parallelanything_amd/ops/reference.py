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


def mod_rows(mod: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """A modulation operand broadcastable against x [B, S, D]: [B, D] gets
    its sequence axis; [B, G, D] with 1 < G < S is the grouped form, row s
    taking modulation row s // (S // G); G = 1 and G = S go as they are."""
    if mod.dim() == x.dim() - 1:
        return mod.unsqueeze(1)
    if mod.dim() == 3 and x.dim() == 3 and mod.shape[1] not in (1, x.shape[1]):
        return mod.repeat_interleave(x.shape[1] // mod.shape[1], dim=1)
    return mod


def check_mod_groups(op: str, x: torch.Tensor, **mods: torch.Tensor) -> None:
    """The refusals of the grouped form, x [B, S, D] beside [B, G, D]
    modulation: S % G != 0 raises ValueError; another B or D, another dtype
    or device than x's, or operands of different shapes RuntimeError, as the
    [B, D] form does."""
    B, S, D = x.shape
    first = None
    for name, m in mods.items():
        G = m.shape[1]
        if (m.shape[0], m.shape[2]) != (B, D):
            raise RuntimeError(f"{op}: {name} must be [B, G, D] = [{B}, G, "
                               f"{D}], got {list(m.shape)}")
        if G < 1 or S % G != 0:
            raise ValueError(f"{op}: S = {S} is not a multiple of G = {G} "
                             f"({name} {list(m.shape)})")
        if m.dtype != x.dtype or m.device != x.device:
            raise RuntimeError(f"{op}: {name} is {m.dtype} on {m.device}, x "
                               f"{x.dtype} on {x.device}")
        if first is not None and m.shape != first[1].shape:
            raise RuntimeError(f"{op}: {first[0]} {list(first[1].shape)} and "
                               f"{name} {list(m.shape)} must have one shape")
        first = first or (name, m)


def layer_norm_mod(
    x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, eps: float = 1e-6
) -> torch.Tensor:
    """AdaLN-modulated LayerNorm: LN(x) * (1 + scale) + shift.

    x: [B, S, D]; scale/shift: [B, D] (broadcast over S), [B, S, D], or the
    grouped [B, G, D] with S % G == 0 (mod_rows).
    No learned affine — modulation plays that role (MMDiT convention).
    """
    dtype = x.dtype
    out = F.layer_norm(_wide(x), (x.shape[-1],), eps=eps)
    scale, shift = mod_rows(scale, x), mod_rows(shift, x)
    out = out * (1.0 + _wide(scale)) + _wide(shift)
    return out.to(dtype)


def gate_residual(residual: torch.Tensor, gate: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """residual + gate * x with gate [B, D] broadcast over sequence, or the
    grouped [B, G, D] (mod_rows)."""
    return residual + mod_rows(gate, x) * x


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


def check_layer_norm(x, weight, bias, residual=None):
    """What no path of ops.layer_norm accepts, raised on every device
    (RuntimeError). The kernel's own limits (16-bit, C % 8 == 0, C <= 2048)
    are not refusals of the op: such inputs run here."""
    def refuse_unless(ok, msg):
        if not ok:
            raise RuntimeError(f"layer_norm: {msg}")

    refuse_unless(x.dim() >= 1, "x must be [..., C]")
    C = x.shape[-1]
    named = [("weight", weight, (C,)), ("bias", bias, (C,))]
    if residual is not None:
        named.append(("residual", residual, tuple(x.shape)))
    for name, t, shape in named:
        refuse_unless(tuple(t.shape) == shape,
                      f"{name} must be {list(shape)}, got {list(t.shape)}")
        refuse_unless(t.dtype == x.dtype,
                      f"{name} dtype ({t.dtype}) must match x ({x.dtype})")
        refuse_unless(t.device == x.device,
                      f"{name} is on {t.device}, x on {x.device}")


def layer_norm(x, weight, bias, eps: float = 1e-5, *, residual=None):
    """Affine LayerNorm over the last dim as nn.LayerNorm computes it, in
    x's dtype. With ``residual``: (s, y), s = residual + x in that dtype and
    y = LayerNorm(s): the residual add and the norm of the UNet's
    TransformerBlock, as the block composes them in eager torch."""
    check_layer_norm(x, weight, bias, residual)
    if residual is None:
        return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    s = residual + x
    return s, F.layer_norm(s, (x.shape[-1],), weight, bias, eps)


def check_geglu(y):
    if y.dim() < 1 or y.shape[-1] % 2:
        raise RuntimeError(f"geglu: y must be [..., 2N], got {list(y.shape)}")


def geglu(y: torch.Tensor) -> torch.Tensor:
    """a * gelu(g), a and g the two halves of the last dim, the erf GELU:
    the UNet's GEGLU as the block composes it in eager torch."""
    check_geglu(y)
    if y.shape[-1] == 0:
        return y.new_empty(y.shape)
    a, g = y.chunk(2, dim=-1)
    return a * F.gelu(g)


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


def as_bool_head_block_mask(mask: torch.Tensor, B: int, H: int, Sq: int,
                            Sk: int) -> torch.Tensor:
    """[Bm, Hm, ceil(Sq/256), ceil(Sk/64)] bool/integer per-head block mask,
    Bm in {1, B}, Hm in {1, H} (nonzero = query block qb of head h of batch
    element b attends the key tile) -> bool. Floating masks are refused for
    as_bool_key_mask's reason; another shape raises ValueError."""
    if mask.dtype.is_floating_point or mask.dtype.is_complex:
        raise ValueError(
            f"block mask must be bool or integer (nonzero = attend), got "
            f"{mask.dtype}: additive float biases are not supported")
    nq, nk = block_mask_shape(Sq, Sk)
    if (mask.dim() != 4 or mask.shape[0] not in (1, B)
            or mask.shape[1] not in (1, H)
            or tuple(mask.shape[2:]) != (nq, nk)):
        raise ValueError(
            f"per-head block mask must be [Bm, Hm, ceil(Sq/{Q_BLOCK}), "
            f"ceil(Sk/{KV_TILE})] = [1 or {B}, 1 or {H}, {nq}, {nk}] for "
            f"B={B}, H={H}, Sq={Sq}, Sk={Sk}, got {list(mask.shape)}")
    return mask if mask.dtype == torch.bool else mask != 0


# Key tiles select_block_mask takes: what one select block of the native
# kernel holds in LDS (ops/hip/block_select.h). 3072 tiles = 196 608 keys.
SELECT_MAX_TILES = 3072


def _block_means(x: torch.Tensor, rows: int) -> torch.Tensor:
    """[B, H, S, D] -> fp64 [B, H, ceil(S/rows), D]: the mean of each block
    of ``rows`` rows, the last one over its rows < S only."""
    B, H, S, D = x.shape
    n = (S + rows - 1) // rows
    xd = torch.nn.functional.pad(x.double(), (0, 0, 0, n * rows - S))
    count = torch.full((n,), rows, dtype=torch.float64, device=x.device)
    if n:
        count[-1] = S - (n - 1) * rows
    return xd.view(B, H, n, rows, D).sum(3) / count[:, None]


def select_scores(q, k, scale: Optional[float] = None):
    """(s, p) of select_block_mask, fp64 [B, H, nq, nk]: the scaled scores of
    the block means and their softmax over the key tiles."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    qbar = _block_means(q, Q_BLOCK)
    kbar = _block_means(k, KV_TILE)
    # a product and a sum per tile, not a matmul: a blocked matmul adds the D
    # terms in an order that depends on the column, so two tiles with the
    # same kbar could differ in the last bit and stop being a tie
    s = scale * torch.stack(
        [(qbar[:, :, i, None, :] * kbar).sum(-1)
         for i in range(qbar.shape[2])], dim=2)
    return s, torch.softmax(s, dim=-1)


def check_select(q, k, top_p, Sq: int, Sk: int):
    """What select_block_mask takes, on every device."""
    if not (q.dim() == 4 and k.dim() == 4):
        raise ValueError(f"select_block_mask expects 4-D q/k, got "
                         f"{q.dim()}-D, {k.dim()}-D")
    if not 0.0 < float(top_p) <= 1.0:
        raise ValueError(f"select_block_mask: top_p must lie in (0, 1], got "
                         f"{top_p}")
    nk = block_mask_shape(Sq, Sk)[1]
    if nk > SELECT_MAX_TILES:
        raise ValueError(
            f"select_block_mask: Sk={Sk} is {nk} key tiles, above the cap of "
            f"{SELECT_MAX_TILES} ({SELECT_MAX_TILES * KV_TILE} keys)")


def select_block_mask(q, k, top_p: float, scale: Optional[float] = None,
                      keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Top-p key tiles per (batch element, head, query block), in fp64: q
    [B, H, Sq, D], k [B, H, Sk, D] -> bool [B, H, ceil(Sq/256), ceil(Sk/64)].

    qbar[b, h, qb] is the mean of the block's query rows < Sq, kbar[b, h, t]
    the mean of the tile's key rows < Sk, s_t = scale * <qbar, kbar_t> and p
    its softmax over t. Tile t is selected iff the total p of the tiles with
    s_u > s_t is < top_p: the shortest descending prefix that reaches mass
    top_p, with ties at the threshold all kept. top_p = 1 selects every tile
    (no summation). ``keep``, an optional [nq, nk] bool/integer block mask,
    is OR-ed in afterwards. This is the mean-pool predictor of SpargeAttn
    without its self-similarity gate; nothing is claimed about quality."""
    Sq, Sk = q.shape[2], k.shape[2]
    check_select(q, k, top_p, Sq, Sk)
    B, H = q.shape[:2]
    nq, nk = block_mask_shape(Sq, Sk)
    if float(top_p) == 1.0 or nq == 0 or nk == 0:
        sel = torch.ones(B, H, nq, nk, dtype=torch.bool, device=q.device)
    else:
        s, p = select_scores(q, k, scale)
        # mass above s_t: the suffix sum of p in ascending order of s, from
        # the first entry greater than s_t
        s_asc, order = torch.sort(s, dim=-1)
        suffix = torch.flip(torch.cumsum(
            torch.flip(torch.gather(p, -1, order), (-1,)), -1), (-1,))
        suffix = torch.nn.functional.pad(suffix, (0, 1))
        first_above = torch.searchsorted(s_asc, s, right=True)
        sel = torch.gather(suffix, -1, first_above) < float(top_p)
    if keep is not None:
        sel = sel | as_bool_block_mask(keep, Sq, Sk).to(q.device)
    return sel


def check_row_bounds(lo, hi, Sq: int):
    """lo, hi: two [Sq] integer tensors (query row i sees the keys lo[i] <=
    j < hi[i]). Floating and bool tensors are refused for as_bool_key_mask's
    reason: nothing is guessed from a mask or a bias. Another rank or length
    raises ValueError."""
    for name, t in (("lo", lo), ("hi", hi)):
        if (t.dtype.is_floating_point or t.dtype.is_complex
                or t.dtype == torch.bool):
            raise ValueError(
                f"row bounds must be integer key indices, got {name} of "
                f"{t.dtype}: masks and additive float biases are not "
                f"supported here")
        if t.dim() != 1 or t.shape[0] != Sq:
            raise ValueError(f"row bounds must be two [Sq] = [{Sq}] tensors, "
                             f"got {name} {list(t.shape)}")
    if lo.device != hi.device:
        raise ValueError(f"row bounds: lo on {lo.device}, hi on {hi.device}")


def as_row_bounds(row_bounds, Sq: int, Sk: int):
    """(lo, hi) checked -> the pair as int64, clamped to [0, Sk]."""
    lo, hi = row_bounds
    check_row_bounds(lo, hi, Sq)
    return lo.long().clamp(0, Sk), hi.long().clamp(0, Sk)


NO_ROW_BOUNDS_WITH_MASK = ("row_bounds= together with key_mask= or "
                           "block_mask= is not supported")


def as_bool_attn_mask(mask: torch.Tensor, B: int, Sq: int,
                      Sk: int) -> torch.Tensor:
    """Dense bool/integer attention mask (nonzero = attend), [Sq, Sk], [Bm,
    Sq, Sk] or [Bm, 1, Sq, Sk] with Bm in {1, B}, shared by heads -> bool
    [Bm, Sq, Sk]. Floating masks are refused for as_bool_key_mask's reason;
    a head dimension other than 1 and any other shape raise ValueError."""
    if mask.dtype.is_floating_point or mask.dtype.is_complex:
        raise ValueError(
            f"attn_mask must be bool or integer (nonzero = attend), got "
            f"{mask.dtype}: additive float biases are not supported")
    shape = tuple(mask.shape)
    if mask.dim() == 4 and shape[1] != 1:
        raise ValueError(
            f"attn_mask is shared by heads: its head dimension must be 1, "
            f"got {list(shape)} (per-head masks are not supported)")
    if mask.dim() == 4:
        mask = mask[:, 0]
    elif mask.dim() == 2:
        mask = mask[None]
    if (mask.dim() != 3 or tuple(mask.shape[1:]) != (Sq, Sk)
            or mask.shape[0] not in (1, B)):
        raise ValueError(
            f"attn_mask must be [Sq, Sk], [Bm, Sq, Sk] or [Bm, 1, Sq, Sk] "
            f"with Sq={Sq}, Sk={Sk} and Bm 1 or {B}, got {list(shape)}")
    return mask if mask.dtype == torch.bool else mask != 0


NO_ATTN_MASK_WITH_MASK = ("attn_mask= together with key_mask=, block_mask= "
                          "or row_bounds= is not supported")


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
    row_bounds=None,
    attn_mask: Optional[torch.Tensor] = None,
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
    zeros. The per-head form is [Bm, Hm, ceil(Sq/256), ceil(Sk/64)] with Bm
    in {1, B} and Hm in {1, H}: block_mask[b or 0][h or 0][i // 256][j // 64]
    under the same contract, K/V rows of head h at keys no query row of that
    (b, h) sees being don't-care.

    row_bounds: optional (lo, hi), two [Sq] integer tensors shared by batch
    and heads. Key j is visible to query row i iff lo[i] <= j < hi[i] and
    j < Sk; the bounds are clamped to [0, Sk], and a row with lo >= hi after
    clamping sees no key and gives zeros. Not supported together with
    key_mask= or block_mask= (ValueError). K/V inside [0, Sk) must be
    finite (see ops.pack_row_bounds).

    attn_mask: optional dense bool/integer mask, [Sq, Sk], [Bm, Sq, Sk] or
    [Bm, 1, Sq, Sk] with Bm in {1, B}, shared by heads. Key j is visible to
    query row i of batch element b iff attn_mask[b or 0][i][j] != 0. A row
    with no visible key gives zeros; K/V rows no query row of the batch
    element sees are don't-care (zeroed before the matmuls). Not supported
    together with any other mask, or with return_lse (ValueError).

    k and v have q's batch, head count and head dim (ValueError otherwise:
    nothing is broadcast, as on the native kernels). Sk = 0 gives zeros.
    """
    check_qkv(q, k, v)
    if attn_mask is not None:
        if not (key_mask is None and block_mask is None
                and row_bounds is None):
            raise ValueError(f"attention: {NO_ATTN_MASK_WITH_MASK}")
        if return_lse:
            raise ValueError("attention: attn_mask= is not supported "
                             "together with the log-sum-exp output")
    if row_bounds is not None and not (key_mask is None
                                       and block_mask is None):
        raise ValueError(f"attention: {NO_ROW_BOUNDS_WITH_MASK}")
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    dtype = q.dtype
    B, Sq, Sk = q.shape[0], q.shape[2], k.shape[2]
    # vis: which keys each query row sees, broadcast over [B, H, Sq, Sk];
    # None = all of them
    vis = None
    if block_mask is not None and block_mask.dim() == 4:
        bm = as_bool_head_block_mask(block_mask, B, q.shape[1], Sq,
                                     Sk).to(q.device)
        vis = bm.repeat_interleave(Q_BLOCK, dim=2).repeat_interleave(
            KV_TILE, dim=3)[:, :, :Sq, :Sk]             # [Bm, Hm, Sq, Sk]
    elif block_mask is not None:
        bm = as_bool_block_mask(block_mask, Sq, Sk).to(q.device)
        vis = bm.repeat_interleave(Q_BLOCK, dim=0).repeat_interleave(
            KV_TILE, dim=1)[None, None, :Sq, :Sk]       # [1, 1, Sq, Sk]
    if key_mask is not None:
        m = as_bool_key_mask(key_mask).to(q.device)
        if m.shape != (B, Sk):
            raise ValueError(f"key mask {tuple(m.shape)} does not match "
                             f"[B={B}, Sk={Sk}]")
        m = m[:, None, None, :]                         # [B, 1, 1, Sk]
        vis = m if vis is None else vis & m
    if row_bounds is not None:
        lo, hi = (t.to(q.device)[:, None]
                  for t in as_row_bounds(row_bounds, Sq, Sk))
        j = torch.arange(Sk, device=q.device)[None, :]
        vis = ((j >= lo) & (j < hi))[None, None]        # [1, 1, Sq, Sk]
    if attn_mask is not None:
        vis = as_bool_attn_mask(attn_mask, B, Sq, Sk).to(
            q.device)[:, None]                          # [Bm, 1, Sq, Sk]
    qf, kf, vf = _wide(q), _wide(k), _wide(v)
    if vis is not None:
        # Unmasked calls skip this: a copy of k or v can take matmul down
        # another path and change bits.
        seen = vis.any(dim=2)[..., None]                # [B|1, 1, Sk, 1]
        kf = torch.where(seen, kf, torch.zeros((), device=k.device))
        vf = torch.where(seen, vf, torch.zeros((), device=v.device))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if vis is not None:
        s = s.masked_fill(~vis, float("-inf"))
    p = torch.softmax(s, dim=-1)
    if vis is not None:
        # a row with no visible key: softmax over all -inf is NaN -> zeros
        p = torch.where(vis.any(dim=3, keepdim=True), p,
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
