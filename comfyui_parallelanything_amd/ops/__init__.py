"""Op dispatch: hand-written gfx950 HIP kernels on GPU, torch reference on CPU.

Policy (deliberate, per the framework's native-code contract):
- Tensors on a HIP device REQUIRE the in-tree native extension `_pa_hip`.
  If it is not importable, ops raise instead of silently falling back to
  eager PyTorch — a GPU run must execute our CDNA4 kernels or fail loudly.
  (Escape hatch for debugging only: PA_ALLOW_EAGER=1.)
- CPU tensors use ops.reference — the same functions that serve as the fp32
  ground truth in the kernel numerics tests.
- Shapes a kernel doesn't cover dispatch to reference WITH a one-time
  warning, so coverage gaps are visible in logs, not silent.

Plain GEMMs (nn.Linear / conv) go through PyTorch-ROCm's hipBLASLt/MIOpen
paths — library GEMMs are the sanctioned exception; the fused/bandwidth
ops here are the hand-written surface.
"""
from __future__ import annotations

import glob
import importlib.util
import logging
import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import reference

log = logging.getLogger("parallelanything.ops")

_EXT = None
_EXT_TRIED = False
_ALLOW_EAGER = os.environ.get("PA_ALLOW_EAGER", "0") == "1"
_WARNED: set = set()
# 16-bit element types with native instantiations of every kernel below
_NATIVE16 = (torch.bfloat16, torch.float16)


def _load_ext():
    global _EXT, _EXT_TRIED
    if _EXT_TRIED:
        return _EXT
    _EXT_TRIED = True
    pkg_dir = os.path.dirname(__file__)
    cands = glob.glob(os.path.join(pkg_dir, "_pa_hip*.so"))
    if not cands:
        return None
    try:
        import torch  # noqa: F401  (must be imported before the ext)

        spec = importlib.util.spec_from_file_location("_pa_hip", cands[0])
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _EXT = mod
        log.info("loaded HIP extension %s", cands[0])
    except Exception as err:  # noqa: BLE001
        log.error("failed to load HIP extension: %r", err)
        _EXT = None
    return _EXT


def hip_ext():
    return _load_ext()


def hip_available(op: Optional[str] = None) -> bool:
    ext = _load_ext()
    if ext is None:
        return False
    return op is None or hasattr(ext, op)


def _require_ext(op: str):
    ext = _load_ext()
    if ext is not None and hasattr(ext, op):
        return ext
    if _ALLOW_EAGER:
        if op not in _WARNED:
            _WARNED.add(op)
            log.warning("PA_ALLOW_EAGER: %s falling back to eager on GPU", op)
        return None
    raise RuntimeError(
        f"HIP extension for op '{op}' is not available on this GPU build — "
        "build it in-tree with `python -m comfyui_parallelanything_amd.ops.build` "
        "(gfx950). Refusing silent eager fallback."
    )


def _unsupported(op: str, why: str):
    key = (op, why)
    if key not in _WARNED:
        _WARNED.add(key)
        log.warning("op %s: shape/dtype not covered by HIP kernel (%s); "
                    "using reference path", op, why)


# ---------------------------------------------------------------------------
# Argument checks of the reference path. The native launchers refuse a call
# whose shapes would make a kernel index outside a tensor (TORCH_CHECK, a
# RuntimeError); the reference path refuses the same calls, so a CPU run
# and a GPU run take the same arguments. docs/KERNELS.md, "Elementwise and
# rotary contract".
# ---------------------------------------------------------------------------

def _refuse_unless(ok: bool, msg: str):
    if not ok:
        raise RuntimeError(msg)


def _check_cs(op: str, cs, S: int, D: int, ref, batched: bool = False):
    want = [S, D // 2, 2]
    ok = list(cs.shape) == want or (
        batched and cs.dim() == 4 and list(cs.shape[1:]) == want)
    _refuse_unless(ok, f"{op}: cs must be [S, D/2, 2] = {want}, got "
                       f"{list(cs.shape)}")
    _refuse_unless(cs.device == ref.device,
                   f"{op}: cs is on {cs.device}, the activations on "
                   f"{ref.device}")


def _check_norm_weight(op: str, name: str, w, D: int, ref):
    _refuse_unless(w.dim() == 1 and w.shape[0] == D,
                   f"{op}: {name} must be [D] = [{D}], got {list(w.shape)}")
    _refuse_unless(w.device == ref.device,
                   f"{op}: {name} is on {w.device}, the activations on "
                   f"{ref.device}")


def _check_qk(q, k, wq, wk, cs):
    op = "qk_norm_rope_"
    _refuse_unless(q.dim() == 4 and k.dim() == 4, f"{op}: [B,S,H,D] views")
    D = q.shape[3]
    _refuse_unless(D % 2 == 0, f"{op}: D must be even, got {D}")
    _refuse_unless(k.shape == q.shape,
                   f"{op}: k {list(k.shape)} must have q's shape "
                   f"{list(q.shape)}")
    _refuse_unless(k.device == q.device,
                   f"{op}: k is on {k.device}, q on {q.device}")
    _check_norm_weight(op, "wq", wq, D, q)
    _check_norm_weight(op, "wk", wk, D, q)
    _check_cs(op, cs, q.shape[1], D, q)


def _check_pack(txt, img, weights, cs):
    op = "pack_joint_qkv"
    _refuse_unless(txt.dim() == 5 and img.dim() == 5,
                   f"{op} expects [B,S,3,H,D] views")
    B, T, _, H, D = txt.shape
    _refuse_unless(D % 2 == 0, f"{op}: D must be even, got {D}")
    _refuse_unless(
        txt.shape[2] == 3 and img.shape[2] == 3
        and (img.shape[0], img.shape[3], img.shape[4]) == (B, H, D),
        f"{op}: txt [B,T,3,H,D] and img [B,Si,3,H,D] must share B, H and D, "
        f"got txt {list(txt.shape)}, img {list(img.shape)}")
    _refuse_unless(img.device == txt.device,
                   f"{op}: img is on {img.device}, txt on {txt.device}")
    for name, w in zip(("wq_t", "wk_t", "wq_i", "wk_i"), weights):
        _check_norm_weight(op, name, w, D, txt)
    _check_cs(op, cs, T + img.shape[1], D, txt)


# ---------------------------------------------------------------------------
# Public ops
# ---------------------------------------------------------------------------

def rms_norm(x: torch.Tensor, weight=None, eps: float = 1e-6) -> torch.Tensor:
    if x.is_cuda:
        ext = _require_ext("rms_norm")
        if ext is not None:
            return ext.rms_norm(x.contiguous(),
                                weight.contiguous() if weight is not None else None,
                                eps)
    return reference.rms_norm(x, weight, eps)


# Limit of the grouped modulation kernels (ops/hip/mod_groups.h): 16 granules
# of 16 bytes a lane
_MOD_GROUPS_MAX_D = 8192


def _mod_groups_native(op: str, x):
    """The extension when the grouped kernels cover x, else None after the
    one-time note (or without one where there is no extension to ask)."""
    ext = _require_ext(op + "_grouped")
    if ext is None:
        return None
    D = x.shape[-1]
    if x.dtype in _NATIVE16 and D % 8 == 0 and D <= _MOD_GROUPS_MAX_D:
        return ext
    _unsupported(op, f"grouped modulation, dtype={x.dtype}, D={D}")
    return None


def layer_norm_mod(x, scale, shift, eps: float = 1e-6) -> torch.Tensor:
    """LN(x) * (1 + scale) + shift over the last dim of x [B, S, D], no
    learned affine. scale and shift are [B, D], one row per batch element,
    or the grouped [B, G, D] with G >= 1 dividing S: row s of batch element
    b takes modulation row [b][s // (S // G)]. G = frames is a timestep per
    latent frame, G = S per-token modulation, G = 1 the [B, D] case in 3-D
    form.

    Grouped calls on the GPU run layer_norm_mod_grouped_kernel for bf16 and
    fp16 with D % 8 == 0 and D <= 8192; anything else there takes the
    reference path with the one-time warning. The modulation is read as it
    is, at any batch and group-row stride (the unbind(-2) views of a [B, G,
    6, D] projection), and copied only when its last dim is not contiguous
    or a row does not start on 16 bytes. Nothing is read on the host.
    Refused on every device: S % G != 0 (ValueError); another B or D, a
    dtype or device other than x's, scale and shift of different shapes
    (RuntimeError). Zero-element inputs return the empty result."""
    grouped = x.dim() == 3 and scale.dim() == 3 and shift.dim() == 3
    if grouped:
        reference.check_mod_groups("layer_norm_mod", x, scale=scale,
                                   shift=shift)
        if x.numel() == 0:
            return torch.empty_like(x)
    if x.is_cuda:
        if grouped:
            ext = _mod_groups_native("layer_norm_mod", x)
            if ext is not None:
                return ext.layer_norm_mod_grouped(x, scale, shift, eps)
            return reference.layer_norm_mod(x, scale, shift, eps)
        ext = _require_ext("layer_norm_mod")
        if ext is not None:
            if scale.dim() == x.dim() - 1:
                # scale/shift go as they are: the launcher reads [B, D]
                # rows at any row stride (column slices of the banked
                # modulation GEMM) and copies only what it cannot read
                return ext.layer_norm_mod(x.contiguous(), scale, shift, eps)
            _unsupported("layer_norm_mod", "per-token modulation")
    return reference.layer_norm_mod(x, scale, shift, eps)


def gate_residual(residual, gate, x) -> torch.Tensor:
    """residual + gate * x; x and residual [B, S, D], gate [B, D] (one row
    per batch element: a broadcast [1, D] gate, another D, or a residual of
    another shape raises) or the grouped [B, G, D] of layer_norm_mod, with
    its coverage, layout rule and refusals (gate_residual_grouped_kernel).
    Zero-element inputs give an empty result."""
    grouped = x.dim() == 3 and gate.dim() == 3
    if grouped:
        reference.check_mod_groups("gate_residual", x, gate=gate)
        _refuse_unless(
            residual.shape == x.shape,
            f"gate_residual: residual {list(residual.shape)} must have x's "
            f"shape {list(x.shape)}")
        _refuse_unless(
            residual.dtype == x.dtype and residual.device == x.device,
            "gate_residual: residual dtype and device must match x's")
        if x.numel() == 0:
            return torch.empty_like(x)
        if x.is_cuda:
            ext = _mod_groups_native("gate_residual", x)
            if ext is not None:
                return ext.gate_residual_grouped(residual, gate, x)
        return reference.gate_residual(residual, gate, x)
    if x.dim() == 3 and gate.dim() == 2 and not x.is_cuda:
        _refuse_unless(
            tuple(gate.shape) == (x.shape[0], x.shape[2]),
            f"gate_residual: gate must be [B, D] = [{x.shape[0]}, "
            f"{x.shape[2]}], got {list(gate.shape)}")
        _refuse_unless(
            residual.shape == x.shape,
            f"gate_residual: residual {list(residual.shape)} must have x's "
            f"shape {list(x.shape)}")
        _refuse_unless(residual.dtype == x.dtype and gate.dtype == x.dtype,
                       "gate_residual: residual and gate dtypes must match "
                       "x's")
    if x.is_cuda:
        ext = _require_ext("gate_residual")
        if ext is not None and gate.dim() == x.dim() - 1:
            # the gate goes as it is, for layer_norm_mod's reason
            return ext.gate_residual(residual.contiguous(), gate,
                                     x.contiguous())
    return reference.gate_residual(residual, gate, x)


def group_norm_silu(x, num_groups: int, weight=None, bias=None,
                    eps: float = 1e-6) -> torch.Tensor:
    if x.is_cuda:
        ext = _require_ext("group_norm_silu")
        if ext is not None:
            if x.dim() == 4 and (x.shape[1] % num_groups) == 0:
                return ext.group_norm_silu(
                    x.contiguous(), int(num_groups),
                    weight.contiguous() if weight is not None else None,
                    bias.contiguous() if bias is not None else None,
                    eps,
                )
            _unsupported("group_norm_silu", f"dim={x.dim()}")
    return reference.group_norm_silu(x, num_groups, weight, bias, eps)


# Limits of the channels-last GroupNorm kernels (ops/hip/group_norm_nhwc.h)
_GN_NHWC_MAX_C = 4096
_GN_NHWC_MAX_GROUPS = 256


def _gn_nhwc_gap(x, num_groups, tensors) -> Optional[str]:
    """Why a GPU call is not covered by the channels-last kernels, or None."""
    if x.dtype not in _NATIVE16:
        return f"dtype={x.dtype}"
    if not x.is_contiguous(memory_format=torch.channels_last):
        return "not dense channels-last"
    C = x.shape[1]
    if C % 8 != 0 or C > _GN_NHWC_MAX_C or num_groups > _GN_NHWC_MAX_GROUPS:
        return f"C={C}, groups={num_groups}"
    if x.data_ptr() % 16 or any(
            t is not None and (not t.is_contiguous() or t.data_ptr() % 16)
            for t in tensors):
        return "strided or unaligned operand"
    return None


def group_norm(x, num_groups: int, weight=None, bias=None, eps: float = 1e-6,
               *, silu: bool = False, channel_add=None) -> torch.Tensor:
    """GroupNorm of x [B, C, H, W], optionally followed by SiLU, of x +
    channel_add when a [B, C] addend is given: it is broadcast over the
    pixels and added in fp32 before the statistics, and the unrounded sum is
    what gets normalised. Returns x's shape, dtype and memory format.

    On the GPU a 16-bit dense channels-last x with C % 8 == 0 (C <= 4096, at
    most 256 groups) runs the channels-last kernels, and the [B, H*W, C]
    token tensor is then a view of the result: ``y.permute(0, 2, 3,
    1).reshape(B, H * W, C)``. Anything else there (NCHW, fp32, odd C) takes
    the reference path with the one-time warning; NCHW models call
    group_norm_silu.

    weight and bias [C], channel_add a contiguous [B, C], all of x's dtype
    on x's device, C a multiple of num_groups: anything else raises
    RuntimeError on every device. B, H or W of zero returns the empty
    result."""
    num_groups = int(num_groups)
    if x.is_cuda:
        ext = _require_ext("group_norm_nhwc")
        if ext is not None:
            reference.check_group_norm(x, num_groups, weight, bias,
                                       channel_add)
            why = _gn_nhwc_gap(x, num_groups, (weight, bias, channel_add))
            if why is None:
                return ext.group_norm_nhwc(x, num_groups, weight, bias,
                                           channel_add, float(eps),
                                           bool(silu), 0)
            _unsupported("group_norm", why)
    return reference.group_norm(x, num_groups, weight, bias, eps, silu=silu,
                                channel_add=channel_add)


# Limit of layer_norm_affine_kernel (ops/hip/token_ops.h): 4 vectors a lane
_LN_AFFINE_MAX_C = 2048


def _dense16(t: torch.Tensor) -> torch.Tensor:
    """t as the token kernels read a dense operand: contiguous, 16-byte
    aligned. Copies only what is neither."""
    if not t.is_contiguous():
        t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def layer_norm(x, weight, bias, eps: float = 1e-5, *, residual=None):
    """Affine LayerNorm over the last dim of x [..., C]. With ``residual``
    (x's shape) it returns (s, y): s = residual + x rounded to x's dtype, the
    new residual stream, and y = LayerNorm(s) of that rounded s, so y is bit
    for bit ``layer_norm(s, ...)``. Without, y alone.

    On the GPU a 16-bit call with C % 8 == 0 and C <= 2048 runs the
    one-wave-per-row kernel (fp32 arithmetic, one rounding per output);
    anything else there (fp32, C = 5120, C % 8) takes the reference path with
    the one-time warning. weight and bias [C] and residual of x's dtype on
    x's device: anything else raises RuntimeError on every device. Zero rows
    return the empty result."""
    reference.check_layer_norm(x, weight, bias, residual)
    if x.is_cuda:
        ext = _require_ext("layer_norm_affine")
        if ext is not None:
            C = x.shape[-1]
            if x.dtype in _NATIVE16 and C % 8 == 0 and 0 < C <= _LN_AFFINE_MAX_C:
                res = ext.layer_norm_affine(
                    _dense16(x).view(-1, C), _dense16(weight), _dense16(bias),
                    None if residual is None
                    else _dense16(residual).view(-1, C), float(eps))
                res = [r.view(x.shape) for r in res]
                return res[0] if residual is None else (res[0], res[1])
            _unsupported("layer_norm", f"dtype={x.dtype}, C={C}")
    return reference.layer_norm(x, weight, bias, eps, residual=residual)


def geglu(y: torch.Tensor) -> torch.Tensor:
    """GEGLU of y [..., 2N] -> [..., N]: a * gelu(g) with a = y[..., :N], g =
    y[..., N:] and the exact erf GELU 0.5 * g * (1 + erf(g / sqrt 2)); NaN in
    is NaN out, and 0 * inf is NaN as in the torch composition.

    On the GPU a 16-bit y with N % 8 == 0 runs the kernel (fp32 arithmetic,
    one rounding), reading in place any view whose last dim is contiguous
    and whose leading dims collapse to rows of one 16-byte-aligned stride (a
    column slice of a wider projection); other views are copied first.
    fp32 or another N takes the reference path with the one-time warning. An
    odd last dim raises RuntimeError on every device."""
    reference.check_geglu(y)
    if y.is_cuda:
        ext = _require_ext("geglu")
        if ext is not None:
            W = y.shape[-1]
            if W == 0:
                return reference.geglu(y)       # empty, nothing to launch
            if y.dtype in _NATIVE16 and W % 16 == 0:
                try:
                    rows = y.view(-1, W)
                except RuntimeError:
                    rows = None
                if rows is None or rows.stride(1) != 1 or rows.data_ptr() % 16 \
                        or (rows.shape[0] > 1 and rows.stride(0) % 8):
                    rows = _dense16(y).view(-1, W)
                return ext.geglu(rows).view(*y.shape[:-1], W // 2)
            _unsupported("geglu", f"dtype={y.dtype}, N={W // 2}")
    return reference.geglu(y)


def rope_apply(x, cs) -> torch.Tensor:
    """Rotate adjacent pairs of x [B, H, S, D] by cs [S, D/2, 2] (cos,
    sin; any floating dtype, any strides). An odd D or another cs shape
    raises."""
    if x.is_cuda:
        ext = _require_ext("rope_apply")
        if ext is not None:
            return ext.rope_apply(x.contiguous(), cs.contiguous())
    _refuse_unless(x.dim() == 4, "rope_apply expects [B, H, S, D]")
    _refuse_unless(x.shape[3] % 2 == 0,
                   f"rope_apply: D must be even, got {x.shape[3]}")
    _check_cs("rope_apply", cs, x.shape[2], x.shape[3], x, batched=True)
    return reference.rope_apply(x, cs.float())


def rope_freqs(positions, dim: int, theta: float = 10000.0) -> torch.Tensor:
    # Table precompute: once per replica per resolution, on the owning GPU
    # (the reference scrubbed these caches off replicas instead —
    # clear_flux_caches, any_device_parallel.py:166-195).
    return reference.rope_freqs(positions, dim, theta)


@dataclass
class KeyMask:
    """A [B, Sk] key-padding mask packed for the masked attention kernels.

    Holds tensors only, so parallel.pipeline's recursive move carries it
    across devices like any other dataclass argument:
      mask   the bool mask, True = attend
      words  [B, ceil(Sk/64)] int64, bit j of word t = key 64*t + j
      live   [B, ceil(Sk/64)] int32, ascending live-tile indices, compacted
      nlive  [B] int32
    On CPU only ``mask`` is set; the reference path needs nothing else.
    """
    mask: torch.Tensor
    words: Optional[torch.Tensor] = None
    live: Optional[torch.Tensor] = None
    nlive: Optional[torch.Tensor] = None


def pack_key_mask(mask) -> KeyMask:
    """Pack a [B, Sk] bool/integer key mask (nonzero = attend) once, for
    any number of attention calls over the same keys.

    Contract of every ``key_mask=`` argument below: only keys are masked;
    K/V rows at masked keys are don't-care (any bit pattern, NaN included);
    a batch element with no live key returns zeros. Floating masks raise —
    additive biases are not supported and 0/1 is never guessed from 0/-inf.
    """
    if isinstance(mask, KeyMask):
        return mask
    m = reference.as_bool_key_mask(mask)
    if m.is_cuda:
        ext = _require_ext("pack_key_mask")
        if ext is not None:
            words, live, nlive = ext.pack_key_mask(m)
            return KeyMask(m, words, live, nlive)
    return KeyMask(m)


def _key_mask_for(key_mask, q) -> KeyMask:
    km = pack_key_mask(key_mask)
    if km.mask.device != q.device:
        raise ValueError(f"key mask on {km.mask.device}, q on {q.device}")
    if km.mask.shape[0] != q.shape[0]:
        raise ValueError(f"key mask batch {km.mask.shape[0]} != q batch "
                         f"{q.shape[0]}")
    if q.is_cuda and km.words is None:
        # packed on CPU (or under PA_ALLOW_EAGER) and moved: pack here
        km = pack_key_mask(km.mask)
    return km


# Block-mask granularity: the attention kernel's own geometry.
ATTN_Q_BLOCK = reference.Q_BLOCK    # 256 query rows per block
ATTN_KV_TILE = reference.KV_TILE    # 64 keys per tile


@dataclass
class BlockMask:
    """A [nq, nk] block mask packed for the block-list attention kernels,
    nq = ceil(Sq/256), nk = ceil(Sk/64), optionally composed with a [B, Sk]
    key mask.

    Tensors, plus the three integers the pack was made for (checked before
    every launch; parallel.pipeline's recursive move carries the tensors
    across devices and leaves the integers as they are):
      block  bool [nq, nk], True = the query block attends the key tile
      keys   optional bool [B, Sk] key mask, True = attend
      words  [B, nk] int64: pack_key_mask's words for ``keys``, or for an
             all-true mask without one (bits at or beyond Sk are 0)
      live   [B, nq, nk] int32: per (b, query block) the ascending tiles t
             with block[qb][t] and words[b][t] != 0, compacted, zero tail
      nlive  [B, nq] int32
    On CPU only ``block`` and ``keys`` are set. ``live`` indexes ``words``
    and drives the kernel's global loads, so the pack kernel is its only
    producer: build one with pack_block_mask, never by hand.

    The per-head form (pack_head_block_mask) holds ``block`` as bool [Bm, Hm,
    nq, nk], Bm in {1, B}, Hm in {1, H}, ``live`` as [B, H, nq, nk], ``nlive``
    as [B, H, nq] and the head count it was packed for in ``heads``, which
    is 0 for the shared form.
    """
    block: torch.Tensor
    keys: Optional[torch.Tensor] = None
    words: Optional[torch.Tensor] = None
    live: Optional[torch.Tensor] = None
    nlive: Optional[torch.Tensor] = None
    batch: int = 0
    Sq: int = 0
    Sk: int = 0
    heads: int = 0


def pack_block_mask(block_mask, batch: int, Sq: int, Sk: int,
                    key_mask=None) -> BlockMask:
    """Pack a [ceil(Sq/256), ceil(Sk/64)] bool/integer block mask (nonzero =
    the 256-row query block attends the 64-key tile) once, for any number of
    attention calls of that batch size and those lengths. The mask is shared
    by all batch elements and heads.

    Contract of every ``block_mask=`` argument below: key j is visible to
    query row i of batch element b iff block_mask[i // 256][j // 64] and (no
    key mask or key_mask[b][j]). A query row with no visible key returns
    zeros. K/V rows at keys that no query block of that batch element sees
    are don't-care (any bit pattern, NaN included). Floating masks raise, as
    in pack_key_mask; another shape raises ValueError. ``key_mask`` is a
    KeyMask or a raw [batch, Sk] mask and becomes part of the pack.
    """
    batch, Sq, Sk = int(batch), int(Sq), int(Sk)
    bm = reference.as_bool_block_mask(block_mask, Sq, Sk)
    keys = _block_mask_keys(key_mask, bm, batch, Sk)
    if bm.is_cuda:
        ext = _require_ext("pack_block_lists")
        if ext is not None:
            words = _block_mask_words(key_mask, keys, bm, batch, Sk)
            live, nlive = ext.pack_block_lists(bm, words)
            return BlockMask(bm, keys, words, live, nlive, batch, Sq, Sk)
    return BlockMask(bm, keys, batch=batch, Sq=Sq, Sk=Sk)


def _block_mask_keys(key_mask, bm, batch: int, Sk: int):
    """The bool [batch, Sk] key mask a block-mask pack composes with, or
    None."""
    if key_mask is None:
        return None
    keys = (key_mask.mask if isinstance(key_mask, KeyMask)
            else reference.as_bool_key_mask(key_mask))
    if tuple(keys.shape) != (batch, Sk):
        raise ValueError(f"key mask {list(keys.shape)} does not match "
                         f"[batch={batch}, Sk={Sk}]")
    if keys.device != bm.device:
        raise ValueError(f"key mask on {keys.device}, block mask on "
                         f"{bm.device}")
    return keys


def _block_mask_words(key_mask, keys, bm, batch: int, Sk: int):
    """pack_key_mask_kernel's words for a block-mask pack: the key mask's, or
    those of an all-true mask."""
    if isinstance(key_mask, KeyMask) and key_mask.words is not None:
        return key_mask.words
    return pack_key_mask(
        keys if keys is not None else
        torch.ones(batch, Sk, dtype=torch.bool, device=bm.device)).words


def pack_head_block_mask(mask, B: int, H: int, Sq: int, Sk: int,
                         key_mask=None) -> BlockMask:
    """Pack a per-head block mask, bool/integer [Bm, Hm, ceil(Sq/256),
    ceil(Sk/64)] with Bm in {1, B} and Hm in {1, H} (nonzero = query block qb
    of head h of batch element b attends the key tile), for attention calls
    of that batch size, head count and lengths. select_block_mask makes one
    from q and k.

    Contract, extending pack_block_mask's: key j is visible to query row i
    of (b, h) iff mask[b or 0][h or 0][i // 256][j // 64] and (no key mask
    or key_mask[b][j]). A row with no visible key returns zeros. K/V rows of
    head h at keys that no query block of that (b, h) sees are don't-care,
    NaN included. Floating masks raise; another shape raises ValueError. A
    broadcast dimension is read through a zero stride, never expanded.

    The result goes into ``block_mask=`` of ops.attention and
    ops.attention_bshd (head dims 40 / 80 zero-padded on the latter, as for
    the shared form). attention_bshd_split and the _lse ops raise
    ValueError: there is no split or lse flavour."""
    B, H, Sq, Sk = int(B), int(H), int(Sq), int(Sk)
    bm = reference.as_bool_head_block_mask(mask, B, H, Sq, Sk)
    keys = _block_mask_keys(key_mask, bm, B, Sk)
    if bm.is_cuda:
        ext = _require_ext("pack_head_block_lists")
        if ext is not None:
            words = _block_mask_words(key_mask, keys, bm, B, Sk)
            live, nlive = ext.pack_head_block_lists(bm, words, H)
            return BlockMask(bm, keys, words, live, nlive, B, Sq, Sk, H)
    return BlockMask(bm, keys, batch=B, Sq=Sq, Sk=Sk, heads=H)


SELECT_MAX_TILES = reference.SELECT_MAX_TILES   # key tiles per select call


def select_block_mask(q, k, top_p: float, *, bshd: bool = False,
                      scale: Optional[float] = None,
                      keep=None) -> torch.Tensor:
    """Per-head block mask from this call's q and k: bool [B, H,
    ceil(Sq/256), ceil(Sk/64)] on q's device, for pack_head_block_mask or
    ``block_mask=``. q and k are [B, H, S, D], or [B, S, H, D] with ``bshd``
    (strided views are read in place).

    Per (b, h, query block) the key tiles are scored by scale * <mean of the
    block's query rows, mean of the tile's key rows> (rows inside Sq / Sk
    only), softmaxed over the tiles, and tile t is selected iff the total
    probability of the tiles scoring above it is < top_p: the shortest
    descending prefix that reaches mass top_p, ties at the threshold all
    kept. top_p lies in (0, 1]; 1 selects every tile and computes nothing.
    ``keep``, an optional [nq, nk] bool/integer block mask (for example
    frame_window_block_mask(frames, T, 0)), is OR-ed in afterwards.
    reference.select_block_mask is the definition, in fp64.

    On the GPU: bf16 / fp16, head dim 64 or 128 natively (other 16-bit head
    dims up to 128 are zero-padded first, which leaves every score as it
    is), rows starting on 16 bytes (RuntimeError otherwise), at most
    SELECT_MAX_TILES key tiles; nothing is read on the host, so select, pack
    and attention capture into one graph. ValueError: top_p outside (0, 1],
    more key tiles than the cap, and on the GPU any other dtype or head dim
    (there is no reference route there).

    This is the mean-pool predictor of SpargeAttn without its
    self-similarity gate. Nothing is claimed about image quality."""
    s_ax, h_ax = (1, 2) if bshd else (2, 1)
    reference.check_select(q, k, top_p, q.shape[s_ax] if q.dim() == 4 else 0,
                           k.shape[s_ax] if k.dim() == 4 else 0)
    B, H, D = q.shape[0], q.shape[h_ax], q.shape[3]
    Sq, Sk = q.shape[s_ax], k.shape[s_ax]
    if (k.shape[0], k.shape[h_ax], k.shape[3]) != (B, H, D):
        raise ValueError(f"select_block_mask: k must have q's batch, heads "
                         f"and head dim, got q {list(q.shape)}, k "
                         f"{list(k.shape)}")
    if k.device != q.device:
        raise ValueError(f"select_block_mask: k on {k.device}, q on "
                         f"{q.device}")
    if keep is not None:
        keep = reference.as_bool_block_mask(keep, Sq, Sk)
        if keep.device != q.device:
            raise ValueError(f"keep mask on {keep.device}, q on {q.device}")
    scale = _softmax_scale(q, scale)
    ext = _require_ext("select_block_mask") if q.is_cuda else None
    if ext is not None:
        if q.dtype not in _NATIVE16 or k.dtype != q.dtype or D > 128:
            raise ValueError(
                f"select_block_mask on the GPU takes bf16 or fp16 q and k of "
                f"one dtype and head dim <= 128, got {q.dtype}, {k.dtype}, "
                f"D={D}")
        nq, nk = reference.block_mask_shape(Sq, Sk)
        if float(top_p) == 1.0 or nq == 0 or nk == 0:
            return torch.ones(B, H, nq, nk, dtype=torch.bool, device=q.device)
        if D not in (64, 128):
            width = 64 if D <= 64 else 128
            q, k = (torch.nn.functional.pad(t, (0, width - D))
                    for t in (q, k))
        return ext.select_block_mask(q, k, float(top_p), scale, bshd, keep)
    if bshd:
        q, k = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3)
    return reference.select_block_mask(q, k, top_p, scale, keep)


def frame_window_block_mask(frames: int, tokens_per_frame: int, window: int,
                            device=None) -> torch.Tensor:
    """Block mask [ceil(S/256), ceil(S/64)], S = frames * tokens_per_frame,
    for video tokens in (frame, row, col) order: a query block attends a key
    tile iff some frame the tile touches lies within ``window`` frames of
    some frame the query block touches.

    Query block i spans frames qlo = 256i // T .. qhi = (min(256(i+1), S) -
    1) // T (T = tokens_per_frame), tile t spans klo .. khi the same way
    with 64, and the block is live iff khi >= qlo - window and klo <= qhi +
    window. That is a block-level superset of "attend frames within
    +-window"; the block mask is the definition."""
    frames, T, window = int(frames), int(tokens_per_frame), int(window)
    if frames < 1 or T < 1 or window < 0:
        raise ValueError(f"frame_window_block_mask: frames={frames}, "
                         f"tokens_per_frame={T}, window={window}")
    S = frames * T
    nq, nk = reference.block_mask_shape(S, S)

    def spans(n, step):
        lo = torch.arange(n, device=device, dtype=torch.int64) * step
        hi = torch.clamp(lo + step, max=S) - 1
        return lo // T, hi // T

    qlo, qhi = spans(nq, ATTN_Q_BLOCK)
    klo, khi = spans(nk, ATTN_KV_TILE)
    return ((khi[None, :] >= qlo[:, None] - window)
            & (klo[None, :] <= qhi[:, None] + window))


def _block_mask_for(block_mask, key_mask, q, Sq: int, Sk: int,
                    H: int) -> BlockMask:
    B = q.shape[0]
    if not isinstance(block_mask, BlockMask):
        if block_mask.device != q.device:
            raise ValueError(f"block mask on {block_mask.device}, q on "
                             f"{q.device}")
        if key_mask is not None:
            key_mask = _key_mask_for(key_mask, q)
        if block_mask.dim() == 4:
            return pack_head_block_mask(block_mask, B, H, Sq, Sk, key_mask)
        return pack_block_mask(block_mask, B, Sq, Sk, key_mask)
    if key_mask is not None:
        raise ValueError("a packed BlockMask takes no separate key_mask=: "
                         "the key mask belongs in the pack "
                         "(pack_block_mask(..., key_mask=))")
    bm = block_mask
    if (bm.batch, bm.Sq, bm.Sk) != (B, Sq, Sk):
        raise ValueError(
            f"BlockMask was packed for (B, Sq, Sk) = "
            f"{(bm.batch, bm.Sq, bm.Sk)}, this call has {(B, Sq, Sk)}")
    if bm.heads and bm.heads != H:
        raise ValueError(f"BlockMask was packed for {bm.heads} heads, this "
                         f"call has {H}")
    if bm.block.device != q.device:
        raise ValueError(f"block mask on {bm.block.device}, q on {q.device}")
    if q.is_cuda and bm.live is None:
        # packed on CPU (or under PA_ALLOW_EAGER) and moved: pack here
        bm = (pack_head_block_mask(bm.block, B, H, Sq, Sk, bm.keys)
              if bm.heads else pack_block_mask(bm.block, B, Sq, Sk, bm.keys))
    return bm


@dataclass
class RowBounds:
    """Per-row key ranges packed for the row-bounds attention kernels: query
    row i sees the keys lo[i] <= j < hi[i], for all batch elements and heads.

    Tensors, plus the two lengths the pack was made for (checked before
    every launch; parallel.pipeline's recursive move carries the tensors
    across devices and leaves the integers as they are):
      lo, hi      the [Sq] integer bounds as given
      lo_c, hi_c  [Sq] int32, clamped to [0, Sk]
      range       [ceil(Sq/256), 4] int32 per query block, in 64-key tiles:
                  t0, t1 the tiles it walks, f0, f1 those every row of it
                  sees whole (ops/hip/attention.h, pack_row_bounds_kernel)
    On CPU only ``lo`` and ``hi`` are set. ``range`` drives the kernel's
    K/V loads, so the pack kernel is its only producer: build one with
    pack_row_bounds, never by hand.
    """
    lo: torch.Tensor
    hi: torch.Tensor
    lo_c: Optional[torch.Tensor] = None
    hi_c: Optional[torch.Tensor] = None
    range: Optional[torch.Tensor] = None
    Sq: int = 0
    Sk: int = 0


def pack_row_bounds(lo, hi, Sq: int, Sk: int) -> RowBounds:
    """Pack per-row key ranges once, for any number of attention calls of
    those lengths: lo and hi are [Sq] integer tensors on q's device, shared
    by all batch elements and heads.

    Contract of every ``row_bounds=`` argument below: key j is visible to
    query row i iff lo[i] <= j < hi[i] and j < Sk. The bounds are clamped to
    [0, Sk] on the device (nothing is read on the host, so pack + attention
    capture into one graph); a row with lo >= hi after clamping sees no key
    and returns zeros. Floating or bool tensors raise, as in pack_key_mask;
    another rank or length raises ValueError. K/V rows at or beyond Sk are
    don't-care, and K/V rows in 64-key tiles that no row of a 256-row query
    block reaches are never loaded for that block; K/V inside [0, Sk) must
    otherwise be finite, because a key one row does not see is still
    multiplied, by p = 0, where another row of its block sees that tile.
    Not supported: together with key_mask= or block_mask=, in
    attention_bshd_split, in the _lse ops (ValueError each), per-head or
    per-batch bounds.
    """
    Sq, Sk = int(Sq), int(Sk)
    reference.check_row_bounds(lo, hi, Sq)
    if lo.is_cuda:
        ext = _require_ext("pack_row_bounds")
        if ext is not None:
            lo_c, hi_c, rng = ext.pack_row_bounds(lo, hi, Sk)
            return RowBounds(lo, hi, lo_c, hi_c, rng, Sq, Sk)
    return RowBounds(lo, hi, Sq=Sq, Sk=Sk)


def causal_row_bounds(Sq: int, Sk: int, device=None):
    """(lo, hi) of causal attention, bottom-right aligned: lo = 0, hi[i] =
    i + 1 + Sk - Sq (the last query row sees every key)."""
    i = torch.arange(int(Sq), device=device, dtype=torch.int64)
    return torch.zeros_like(i), i + (1 + int(Sk) - int(Sq))


def frame_span_row_bounds(frames: int, tokens_per_frame: int, back, ahead: int,
                          device=None):
    """(lo, hi) for video tokens in (frame, row, col) order, S = frames *
    tokens_per_frame: the token of frame f sees exactly the frames f - back
    .. f + ahead, lo[i] = max(0, f - back) * T and hi[i] = min(frames, f +
    ahead + 1) * T with f = i // T. back=None reaches every earlier frame
    (lo = 0): (None, 0) is frame-causal attention, (W, W) the +-W window."""
    frames, T, ahead = int(frames), int(tokens_per_frame), int(ahead)
    if frames < 1 or T < 1 or ahead < 0 or (back is not None and back < 0):
        raise ValueError(f"frame_span_row_bounds: frames={frames}, "
                         f"tokens_per_frame={T}, back={back}, ahead={ahead}")
    f = torch.arange(frames * T, device=device, dtype=torch.int64) // T
    lo = (torch.zeros_like(f) if back is None
          else torch.clamp(f - int(back), min=0) * T)
    return lo, torch.clamp(f + ahead + 1, max=frames) * T


def _row_bounds_for(row_bounds, q, Sq: int, Sk: int) -> RowBounds:
    rb = row_bounds
    if not isinstance(rb, RowBounds):
        rb = pack_row_bounds(*rb, Sq, Sk)
    elif (rb.Sq, rb.Sk) != (Sq, Sk):
        raise ValueError(f"RowBounds was packed for (Sq, Sk) = "
                         f"{(rb.Sq, rb.Sk)}, this call has {(Sq, Sk)}")
    if rb.lo.device != q.device or rb.hi.device != q.device:
        raise ValueError(f"row bounds on {rb.lo.device}, q on {q.device}")
    if q.is_cuda and rb.range is None:
        # packed on CPU (or under PA_ALLOW_EAGER) and moved: pack here
        rb = pack_row_bounds(rb.lo, rb.hi, Sq, Sk)
    return rb


_NO_ROW_BOUNDS = ("row_bounds= is not supported in {} (attention and "
                  "attention_bshd take it)")


@dataclass
class AttnMask:
    """A dense attention mask packed for the dense-mask attention kernels:
    query row i of batch element b sees an arbitrary set of keys, shared by
    heads.

    Tensors, plus the three integers the pack was made for (checked before
    every launch; parallel.pipeline's recursive move carries the tensors
    across devices and leaves the integers as they are). With nq =
    ceil(Sq/256), nk = ceil(Sk/64) and Bm = 1 (shared by the batch) or batch:
      mask   bool [Bm, Sq, Sk], True = attend
      bits   [Bm, nk, Sq] int64: bit j of bits[bm][t][i] = mask[bm][i][64t+j]
      words  [Bm, nq, nk] int64: OR of the block's rows' words, the K/V rows
             the block stages
      list   [Bm, nq, nk] int32: per (bm, query block) the ascending tiles
             with a nonzero OR word, compacted, zero tail; bit 30 of an entry
             is set when every row of the block sees the tile whole
      nlist  [Bm, nq] int32
    On CPU only ``mask`` is set. ``list`` drives the kernel's K/V loads, so
    the pack kernels are its only producers: build one with pack_attn_mask,
    never by hand (ops/hip/attention.h, pack_attn_mask_kernel).
    """
    mask: torch.Tensor
    bits: Optional[torch.Tensor] = None
    words: Optional[torch.Tensor] = None
    list: Optional[torch.Tensor] = None
    nlist: Optional[torch.Tensor] = None
    batch: int = 0
    Sq: int = 0
    Sk: int = 0


def pack_attn_mask(mask, batch: int, Sq: int, Sk: int) -> AttnMask:
    """Pack a dense bool/integer attention mask (nonzero = attend) once, for
    any number of attention calls of that batch size and those lengths:
    [Sq, Sk], [Bm, Sq, Sk] or [Bm, 1, Sq, Sk] with Bm in {1, batch}, shared
    by heads. What torch SDPA and ComfyUI's optimized_attention call a
    boolean attn_mask.

    Contract of every ``attn_mask=`` argument below: key j is visible to
    query row i of batch element b iff mask[b or 0][i][j] != 0 and j < Sk. A
    row with no visible key returns zeros exactly. A 256-row query block
    loads only the K/V rows some row of it sees: K/V rows that no query row
    of the batch element sees are don't-care (NaN included), every other K/V
    row must be finite, because a key one row does not see still meets p = 0
    where another row of its block sees it. Nothing is read on the host, so
    pack + attention capture into one graph. Floating masks raise, as in
    pack_key_mask; a head dimension other than 1 or another shape raises
    ValueError. Not supported: together with key_mask=, block_mask= or
    row_bounds=, in the _lse ops (ValueError each), per-head masks, additive
    biases. Head dims 40 / 80 follow the block masks' rule (attention_bshd).

    Cost: the bool mask is Sq * Sk bytes per batch element and the pack 1/8
    of it (2.6 MB at S = 4608). A mask too large to hold as a dense bool
    tensor (WAN's 75k tokens: 5.7 GB) is out of scope: use block_mask= or
    row_bounds= there.
    """
    batch, Sq, Sk = int(batch), int(Sq), int(Sk)
    m = reference.as_bool_attn_mask(mask, batch, Sq, Sk)
    if m.is_cuda:
        ext = _require_ext("pack_attn_mask")
        if ext is not None:
            return AttnMask(m, *ext.pack_attn_mask(m), batch, Sq, Sk)
    return AttnMask(m, batch=batch, Sq=Sq, Sk=Sk)


def _attn_mask_for(attn_mask, q, Sq: int, Sk: int) -> AttnMask:
    B = q.shape[0]
    am = attn_mask
    if not isinstance(am, AttnMask):
        am = pack_attn_mask(am, B, Sq, Sk)
    elif (am.batch, am.Sq, am.Sk) != (B, Sq, Sk):
        raise ValueError(
            f"AttnMask was packed for (B, Sq, Sk) = "
            f"{(am.batch, am.Sq, am.Sk)}, this call has {(B, Sq, Sk)}")
    if am.mask.device != q.device:
        raise ValueError(f"attn_mask on {am.mask.device}, q on {q.device}")
    if q.is_cuda and am.bits is None:
        # packed on CPU (or under PA_ALLOW_EAGER) and moved: pack here
        am = pack_attn_mask(am.mask, B, Sq, Sk)
    return am


_NO_ATTN_MASK_LSE = ("attn_mask= is not supported together with the "
                     "log-sum-exp output (attention_lse / attention_bshd_lse "
                     "take key_mask= only)")


def _mask_for(key_mask, block_mask, q, Sq: int, Sk: int, row_bounds=None,
              attn_mask=None, H: int = 0):
    """The call's packed mask: None, a KeyMask, a BlockMask (which holds
    the key mask too), a RowBounds or an AttnMask. H: the call's head
    count, which a per-head block mask is checked against."""
    if attn_mask is not None:
        if not (key_mask is None and block_mask is None
                and row_bounds is None):
            raise ValueError(
                f"attention: {reference.NO_ATTN_MASK_WITH_MASK}")
        return _attn_mask_for(attn_mask, q, Sq, Sk)
    if row_bounds is not None:
        if key_mask is not None or block_mask is not None:
            raise ValueError(
                f"attention: {reference.NO_ROW_BOUNDS_WITH_MASK}")
        return _row_bounds_for(row_bounds, q, Sq, Sk)
    if block_mask is not None:
        return _block_mask_for(block_mask, key_mask, q, Sq, Sk, H)
    return None if key_mask is None else _key_mask_for(key_mask, q)


def _mask_kw(km) -> dict:
    """``km`` as keyword arguments of reference.attention / ops.attention*."""
    if isinstance(km, BlockMask):
        return {"key_mask": km.keys, "block_mask": km.block}
    if isinstance(km, RowBounds):
        return {"row_bounds": (km.lo, km.hi)}
    if isinstance(km, AttnMask):
        return {"attn_mask": km.mask}
    return {"key_mask": None if km is None else km.mask}


def _softmax_scale(q, scale: Optional[float]) -> float:
    """The call's softmax scale: 1/sqrt(D) by default, else ``scale``, which
    must be positive. The native kernels track the raw score maximum and
    apply the scale afterwards ("max commutes with a positive scale"), and
    their dead-key sentinel is a large negative raw score: with scale < 0
    the running maximum is the scaled minimum and the output is inf/NaN,
    with scale == 0 dead keys of a partial tile weigh as much as live ones.
    Refused on every device, so CPU and GPU runs take the same arguments."""
    if scale is None:
        return 1.0 / math.sqrt(q.shape[-1])
    scale = float(scale)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"attention scale must be positive and finite, "
                         f"got {scale}")
    return scale


_check_qkv = reference.check_qkv


def _attn_op(bshd: bool, split=None, lse: bool = False) -> str:
    """attn_fwd[_bshd][_split][_lse]: the op as _unsupported names it, and
    the extension's binding up to its _masked / _band / _bits suffix."""
    return ("attn_fwd" + ("_bshd" if bshd else "")
            + ("_split" if split is not None else "")
            + ("_lse" if lse else ""))


def _attn_head_dim(ext, q, km, bshd: bool, split=None, lse: bool = False):
    """The head-dim rule: the head dim the kernels run this call at. That
    is D itself for 64 and 128 (the two tile classes, in every flavour) and
    for the other head dims of the extension's table (40, 80) on plain and
    key-masked calls; 64 or 128, to zero-pad to, for what is left of the
    16-bit head dims under 128 on the un-split BSHD ops (see attention_bshd);
    None when the call is not covered. Row bounds and dense masks follow the
    block masks' rule: 40 and 80 are padded."""
    D = q.shape[-1]
    if q.dtype not in _NATIVE16:
        return None
    plain = (split is None and not lse
             and not isinstance(km, (BlockMask, RowBounds, AttnMask)))
    if D in (64, 128) or (plain and D in ext.attn_native_head_dims()):
        return D
    if D < 128 and bshd and split is None:
        return 64 if D <= 64 else 128
    return None


def _attn_native(q, k, v, scale: float, km, bshd: bool,
                 split: Optional[int] = None, lse: bool = False):
    """One attention call on the native kernels: (result, None), or
    (None, why) when the call is not covered. ``why`` is None when there
    is no extension to ask (PA_ALLOW_EAGER). ``result`` is the output, the
    two outputs with ``split``, (out, lse) with ``lse``.

    Picks ext.attn_fwd[_bshd][_split][_lse][_masked]; ``km`` is None, a
    KeyMask, a BlockMask, whose 3-D ``live`` selects the block-list
    kernels inside the masked entry points and whose 4-D ``live`` their
    per-head flavour, a RowBounds, which has the
    _band entry points, or an AttnMask, which has the _bits ones."""
    band, bits = isinstance(km, RowBounds), isinstance(km, AttnMask)
    name = _attn_op(bshd, split, lse) + (
        "_band" if band else "_bits" if bits
        else "_masked" if km is not None else "")
    ext = _require_ext(name)
    if ext is None:
        return None, None
    D = q.shape[-1]
    width = _attn_head_dim(ext, q, km, bshd, split, lse)
    if width is None:
        return None, f"dtype={q.dtype}, D={D}"
    args = (float(scale),)
    if split is not None:
        args += (int(split),)
    if band:
        args += (km.lo_c, km.hi_c, km.range)
    elif bits:
        args += (km.bits, km.words, km.list, km.nlist)
    elif km is not None:
        args += (km.words, km.live, km.nlive)
    if width != D:
        q, k, v = (torch.nn.functional.pad(t, (0, width - D))
                   for t in (q, k, v))
    elif not bshd:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    res = getattr(ext, name)(q, k, v, *args)
    if width == D:
        return (tuple(res) if lse or split is not None else res), None
    # padding q and k leaves every score, so the lse, unchanged; the padded
    # v columns come off the output
    return ((res[0][..., :D], res[1]) if lse else res[..., :D]), None


def _attention(q, k, v, scale, key_mask, block_mask, *, bshd: bool,
               split: Optional[int] = None, lse: bool = False,
               row_bounds=None, attn_mask=None):
    """The body of the five public ops: check, pack the mask, run the native
    kernels, else note the gap and take the reference path."""
    Sq, Sk = _check_qkv(q, k, v, bshd=bshd, split=split)
    scale = _softmax_scale(q, scale)
    km = _mask_for(key_mask, block_mask, q, Sq, Sk, row_bounds, attn_mask,
                   H=q.shape[2 if bshd else 1])
    if isinstance(km, BlockMask) and km.heads and split is not None:
        raise ValueError("attention_bshd_split: per-head block masks have "
                         "no split flavour (attention and attention_bshd "
                         "take them)")
    why = None
    if q.is_cuda:
        res, why = _attn_native(q, k, v, scale, km, bshd, split, lse)
        if res is not None:
            return res
    if split is not None:
        # Composed from the un-split op, which is also how a split call
        # reaches the native head dims and the zero-pad route: that is no
        # reference-path fallback. One that is, is noted here (unmasked
        # calls only) and by the un-split op.
        if (why is not None and km is None
                and _attn_head_dim(hip_ext(), q, km, bshd) is None):
            _unsupported(_attn_op(bshd, split), why)
        if isinstance(km, AttnMask):
            out = _attention(q, k, v, scale, None, None, bshd=bshd,
                             attn_mask=km)
        else:
            packed = (None, km) if isinstance(km, BlockMask) else (km, None)
            out = _attention(q, k, v, scale, *packed, bshd=bshd)
        return out[:, :split].contiguous(), out[:, split:].contiguous()
    if why is not None:
        _unsupported(_attn_op(bshd, lse=lse), why)
    if bshd:
        q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    res = reference.attention(q, k, v, scale, return_lse=lse, **_mask_kw(km))
    if not bshd:
        return res
    if not lse:
        return res.permute(0, 2, 1, 3)
    return res[0].permute(0, 2, 1, 3), res[1].permute(0, 2, 1).contiguous()


def attention(q, k, v, scale: Optional[float] = None,
              key_mask=None, block_mask=None, row_bounds=None,
              attn_mask=None) -> torch.Tensor:
    """Flash-style fused attention, layout [B, H, S, D].

    key_mask: optional KeyMask or raw [B, Sk] bool/integer mask (see
    pack_key_mask for the contract).
    block_mask: optional BlockMask or raw [ceil(Sq/256), ceil(Sk/64)]
    bool/integer mask (see pack_block_mask for the contract). A raw one is
    packed per call, together with key_mask; a packed one already holds its
    key mask, and passing key_mask= beside it raises. The per-head form, a
    raw [Bm, Hm, nq, nk] mask (Bm in {1, B}, Hm in {1, H}) or what
    pack_head_block_mask returns, goes here too (see pack_head_block_mask
    and select_block_mask); attention_bshd_split refuses it.
    row_bounds: optional RowBounds or raw (lo, hi) pair of [Sq] integer
    tensors, query row i seeing the keys lo[i] <= j < hi[i] (see
    pack_row_bounds for the contract; causal_row_bounds and
    frame_span_row_bounds build the usual ones). A raw pair is packed per
    call. Together with key_mask= or block_mask= it raises ValueError.
    attn_mask: optional AttnMask or raw dense bool/integer mask, [Sq, Sk],
    [Bm, Sq, Sk] or [Bm, 1, Sq, Sk] with Bm in {1, B}: query row i of batch
    element b sees the keys j with mask[b or 0][i][j] != 0 (see
    pack_attn_mask for the contract and the memory cost). A raw one is
    packed per call. Together with any other mask it raises ValueError.

    k and v have q's batch, head count and head dim and one length Sk;
    anything else raises ValueError (nothing is broadcast). B, H or Sq of
    zero returns the empty result, Sk = 0 zeros: no row sees a key."""
    return _attention(q, k, v, scale, key_mask, block_mask, bshd=False,
                      row_bounds=row_bounds, attn_mask=attn_mask)


def attention_bshd(q, k, v, scale: Optional[float] = None,
                   key_mask=None, block_mask=None,
                   row_bounds=None, attn_mask=None) -> torch.Tensor:
    """Fused attention on [B, S, H, D] (strided views allowed — e.g. slices
    of a fused qkv projection; no transpose/contiguous copies on GPU).

    key_mask: optional KeyMask or raw [B, Sk] bool/integer mask (see
    pack_key_mask for the contract). block_mask: optional BlockMask or raw
    [ceil(Sq/256), ceil(Sk/64)] mask, row_bounds: optional RowBounds or raw
    (lo, hi) pair, attn_mask: optional AttnMask or raw dense mask, all as in
    attention.

    Head dims. 64 and 128 are the kernel's two tile classes. SD1.5's 40 and
    80 have kernels of their own inside those classes (docs/KERNELS.md,
    "Native head dims"), here and in ops.attention, plain or with key_mask=:
    no pad, no copy, a contiguous output, and bit for bit what the zero-pad
    route gave. Their views must start every row on 16 bytes (any slice of a
    fused qkv projection does); one that does not raises RuntimeError.

    Cost statement for what still pads. Other 16-bit head dims under 128
    (48, 72, 88, 96, ...), and 40 / 80 with block_mask=, row_bounds= or
    attn_mask=, in
    attention_bshd_split and in the _lse ops, are zero-padded up to 64 / 128
    on this op: padding q/k leaves every softmax score unchanged, padded v
    columns are sliced off the output. That wastes attention FLOPs in
    proportion to the padded dim (60 % at 40 -> 64 and 80 -> 128) and costs
    one pad copy each of q, k, v, and the caller's .flatten(2) copies the
    sliced output once more. One more native head dim is one line of the
    extension's table plus its instantiations. Head dims above 128 (160)
    need a 256-class tile that does not exist: they take the reference path
    with a warning.
    """
    return _attention(q, k, v, scale, key_mask, block_mask, bshd=True,
                      row_bounds=row_bounds, attn_mask=attn_mask)


def attention_bshd_split(q, k, v, split: int, scale: Optional[float] = None,
                         key_mask=None, block_mask=None, row_bounds=None,
                         attn_mask=None):
    """attention_bshd with per-stream outputs: rows [:split] and [split:]
    land in two contiguous tensors (feeds dual-stream projections with no
    reshape copies). key_mask, block_mask and attn_mask as in
    attention_bshd; row_bounds= raises ValueError: not supported here."""
    if row_bounds is not None:
        raise ValueError(_NO_ROW_BOUNDS.format("attention_bshd_split"))
    return _attention(q, k, v, scale, key_mask, block_mask, bshd=True,
                      split=split, attn_mask=attn_mask)


_NO_BLOCK_LSE = ("block masks are not supported together with the "
                 "log-sum-exp output (attention_lse / attention_bshd_lse take "
                 "key_mask= only)")


def attention_lse(q, k, v, scale: Optional[float] = None, key_mask=None,
                  block_mask=None, row_bounds=None, attn_mask=None):
    """attention that also returns the log-sum-exp: (out [B, H, Sq, D], fp32
    lse [B, H, Sq]), lse = log of the sum over the row's visible keys of
    exp(scale * q.k). Partial results over disjoint key sets combine exactly
    through it (attention_merge).

    Arguments, refusals and empties as in attention; a row that sees no key
    (Sk = 0, a batch element with no live key) has out = 0 and lse = -inf.
    block_mask=, row_bounds= and attn_mask= raise ValueError: none is
    supported with the lse."""
    if attn_mask is not None:
        raise ValueError(f"attention_lse: {_NO_ATTN_MASK_LSE}")
    if row_bounds is not None:
        raise ValueError(_NO_ROW_BOUNDS.format("attention_lse"))
    if block_mask is not None:
        raise ValueError(f"attention_lse: {_NO_BLOCK_LSE}")
    return _attention(q, k, v, scale, key_mask, None, bshd=False, lse=True)


def attention_bshd_lse(q, k, v, scale: Optional[float] = None, key_mask=None,
                       block_mask=None, row_bounds=None, attn_mask=None):
    """attention_bshd that also returns the log-sum-exp: (out [B, Sq, H, D],
    fp32 lse [B, Sq, H]); see attention_lse. Strided views and head dims
    under 128 work as in attention_bshd."""
    if attn_mask is not None:
        raise ValueError(f"attention_bshd_lse: {_NO_ATTN_MASK_LSE}")
    if row_bounds is not None:
        raise ValueError(_NO_ROW_BOUNDS.format("attention_bshd_lse"))
    if block_mask is not None:
        raise ValueError(f"attention_bshd_lse: {_NO_BLOCK_LSE}")
    return _attention(q, k, v, scale, key_mask, None, bshd=True, lse=True)


ATTN_MERGE_MAX = reference.MERGE_MAX    # partials per merge: a node's GPUs


def attention_merge(outs, lses, return_lse: bool = False):
    """Combine N partial attention results over disjoint key sets into the
    result over their union, exactly, through their log-sum-exp.

    outs: 1 to 8 tensors [..., D] of one shape, dtype (bf16 or fp16 on the
    GPU) and device, D a multiple of 8 there; lses: the N matching fp32
    [...] tensors, as attention_lse / attention_bshd_lse return them. Per
    row, in fp32: m = max_c lse_c; w_c = exp(lse_c - m); out = (sum_c w_c
    out_c) / sum_c w_c, rounded once; lse = m + log sum_c w_c. A partial
    with lse_c = -inf is skipped, so its out_c is don't-care (NaN included);
    all of them -inf gives out = +0, lse = -inf. N = 1 returns the partial
    bit for bit. Returns out, or (out, lse) with return_lse.

    N outside 1..8 raises ValueError; another shape, dtype or device among
    the partials, or an lse that is not fp32, raises RuntimeError on every
    device."""
    outs, lses = list(outs), list(lses)
    reference.check_merge(outs, lses)
    o0 = outs[0]
    if o0.is_cuda:
        ext = _require_ext("attn_merge")
        if ext is not None:
            if o0.dtype in _NATIVE16 and o0.shape[-1] % 8 == 0 \
                    and o0.shape[-1] > 0:
                res = ext.attn_merge([o.contiguous() for o in outs],
                                     [l.contiguous() for l in lses],
                                     bool(return_lse))
                return tuple(res) if return_lse else res[0]
            _unsupported("attn_merge", f"dtype={o0.dtype}, D={o0.shape[-1]}")
    return reference.attention_merge(outs, lses, return_lse)


def qk_norm_rope_(q, k, wq, wk, cs, eps: float = 1e-6):
    """In-place fused qk RMSNorm + RoPE on [B, S, H, D] views.

    Replaces four bandwidth passes (rms q, rms k, rope q, rope k) with one;
    per-replica cs tables live on the owning GPU (see models.layers).
    """
    if q.is_cuda:
        ext = _require_ext("qk_norm_rope_")
        if ext is not None and q.dtype in _NATIVE16 and q.shape[-1] <= 128:
            ext.qk_norm_rope_(q, k, wq, wk, cs, eps)
            return q, k
        _unsupported("qk_norm_rope_", f"dtype={q.dtype}, D={q.shape[-1]}")
    _check_qk(q, k, wq, wk, cs)
    # fp32 throughout, one rounding at the end, as the kernel does: rounding
    # the normalised row to 16 bits first costs whole spacings wherever the
    # rotation cancels
    # (fp64 views stay fp64: reference._wide)
    wide = reference._wide
    cs = wide(cs)
    qn = reference.rms_norm(wide(q), wide(wq), eps).permute(0, 2, 1, 3)
    kn = reference.rms_norm(wide(k), wide(wk), eps).permute(0, 2, 1, 3)
    q.copy_(reference.rope_apply(qn, cs).permute(0, 2, 1, 3))
    k.copy_(reference.rope_apply(kn, cs).permute(0, 2, 1, 3))
    return q, k


def pack_joint_qkv(txt_qkv, img_qkv, wq_t, wk_t, wq_i, wk_i, cs,
                   eps: float = 1e-6):
    """Dual-stream joint qkv pack: per-stream qk RMSNorm + RoPE + contiguous
    [B, T+Si, H, D] q/k/v in one pass (txt_qkv/img_qkv: [B,S,3,H,D] views).

    The two streams share B, H and D and may differ in every stride; T or
    Si may be 0; the four weights are [D], cs [T+Si, D/2, 2]. Anything else
    raises before the launch. v is copied bit for bit."""
    if txt_qkv.is_cuda:
        ext = _require_ext("pack_joint_qkv")
        if ext is not None and txt_qkv.dtype in _NATIVE16 \
                and txt_qkv.shape[-1] <= 128:
            return ext.pack_joint_qkv(txt_qkv, img_qkv, wq_t, wk_t, wq_i, wk_i,
                                      cs, eps)
        _unsupported("pack_joint_qkv",
                     f"dtype={txt_qkv.dtype}, D={txt_qkv.shape[-1]}")
    _check_pack(txt_qkv, img_qkv, (wq_t, wk_t, wq_i, wk_i), cs)
    T = txt_qkv.shape[1]
    tq, tk, tv = txt_qkv.unbind(2)
    iq, ik, iv = img_qkv.unbind(2)
    qk_norm_rope_(tq, tk, wq_t, wk_t, cs[:T], eps)
    qk_norm_rope_(iq, ik, wq_i, wk_i, cs[T:], eps)
    q = torch.cat([tq, iq], dim=1)
    k = torch.cat([tk, ik], dim=1)
    v = torch.cat([tv, iv], dim=1)
    return q, k, v


def quant_fp8(x: torch.Tensor, scale: torch.Tensor,
              amax_buf: torch.Tensor,
              scale_used: torch.Tensor | None = None) -> torch.Tensor:
    """Fused bf16 -> e4m3fn cast with running-amax update (delayed scaling).

    The fused epilogue overwrites ``scale[0]`` with the NEXT call's scale;
    pass a separate ``scale_used`` buffer to receive a snapshot of the scale
    this call actually quantized with (what _scaled_mm must dequantize by).
    GPU-only; used by the fp8 serving mode.

    The emit contract, shared with ``gelu_fp8`` and ``layer_norm_mod_fp8``
    (docs/KERNELS.md, "fp8 emit contract"): ``out = e4m3fn(y * fp32(1 /
    scale[0]))``, rounded to nearest even (subnormal codes included, ``-0``
    kept), saturated to +-448; ``+-inf`` gives +-448 and NaN a NaN byte.
    With a two-slot ``amax_buf``: ``scale_used = scale``; ``amax_buf[0] =
    max(amax_buf[0], max|y|) * 0.999``; ``scale = max(amax_buf[0] / 448,
    1e-12)``, each one fp32 operation. NaN never enters the amax. When the
    running amax is not finite (an inf activation) the scale stays as it
    was and ``amax_buf[0] = scale * 448``, so one inf costs one saturated
    call and not the layer. A one-slot ``amax_buf`` only takes the max."""
    ext = _require_ext("quant_fp8")
    return ext.quant_fp8(x, scale, amax_buf,
                         scale if scale_used is None else scale_used)


def gelu_fp8(x, scale, amax_buf, scale_used) -> torch.Tensor:
    """tanh-GELU emitting e4m3fn with quant_fp8's emit and delayed-scaling
    contract (fp8 serving mode: the MLP-down GEMM consumes the output
    directly, no standalone quant pass): NaN in is a NaN byte out, +inf
    saturates to 448. GPU-only."""
    ext = _require_ext("gelu_fp8")
    return ext.gelu_fp8(x, scale, amax_buf, scale_used)


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        ext = _require_ext("gelu_tanh")
        if ext is not None:
            return ext.gelu_tanh(x)
    return torch.nn.functional.gelu(x, approximate="tanh")


def timestep_embedding(t, dim: int, max_period: float = 10000.0,
                       time_factor: float = 1000.0) -> torch.Tensor:
    """Sinusoidal embedding of t [B] -> fp32 [B, dim], cos | sin halves and
    a zero last column when dim is odd (dim = 1 is that column alone).

    Domain: any fp32 argument t * time_factor; the cos / sin are range-
    reduced library functions, not the hardware instructions that stop at
    256 revolutions. Each output is within 1.5e-7 + 36.8 * |arg| * 2^-24 of
    the fp64 value at arg = t * time_factor * freq_j, checked up to |arg| =
    2e4 (docs/KERNELS.md, "Elementwise and rotary contract")."""
    if t.dim() != 1:
        raise RuntimeError(f"timestep_embedding: t [B], got {list(t.shape)}")
    if t.is_cuda:
        ext = _require_ext("timestep_embedding")
        if ext is not None:
            return ext.timestep_embedding(t.contiguous().float(), int(dim),
                                          float(max_period), float(time_factor))
    return reference.timestep_embedding(t, dim, max_period, time_factor)


def layer_norm_mod_fp8(x, scale, shift, qscale, amax_buf, scale_used,
                       eps: float = 1e-6) -> torch.Tensor:
    """AdaLN-modulated LayerNorm emitting e4m3fn directly (fp8 serving
    mode): the bf16->fp8 cast fuses into the normalize pass, replacing
    layer_norm_mod + quant_fp8 (two HBM round-trips -> one). Delayed
    scaling matches quant_fp8: quantizes with qscale[0], updates the
    running amax, writes the next scale, snapshots the used scale into
    scale_used; a row that holds a NaN comes out as NaN bytes and leaves
    the amax alone. ``scale`` and ``shift`` must be [B, D] tensors of x's
    dtype on x's device (anything else raises before the launch).
    GPU-only."""
    ext = _require_ext("layer_norm_mod_fp8")
    return ext.layer_norm_mod_fp8(x, scale, shift, qscale, amax_buf,
                                  scale_used, float(eps))


def timestep_embed_mlp(t, w1, b1, max_period: float = 10000.0,
                       time_factor: float = 1000.0) -> torch.Tensor:
    """Fused sinusoidal embedding + first Linear + SiLU: [B] -> [B, H].

    SURVEY §2b timestep-MLP fusion (the in_layer half; the out Linear is a
    GEMM and stays on hipBLASLt). GPU-only — callers fall back to the
    composed path on CPU (MLPEmbedder.forward_timestep). The sinusoid has
    timestep_embedding's argument domain and error bound."""
    ext = _require_ext("timestep_embed_mlp")
    return ext.timestep_embed_mlp(t, w1, b1, float(max_period),
                                  float(time_factor))
