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


def layer_norm_mod(x, scale, shift, eps: float = 1e-6) -> torch.Tensor:
    if x.is_cuda:
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
    another shape raises). Zero-element inputs give an empty result."""
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
    """
    block: torch.Tensor
    keys: Optional[torch.Tensor] = None
    words: Optional[torch.Tensor] = None
    live: Optional[torch.Tensor] = None
    nlive: Optional[torch.Tensor] = None
    batch: int = 0
    Sq: int = 0
    Sk: int = 0


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
    keys = None
    if key_mask is not None:
        keys = (key_mask.mask if isinstance(key_mask, KeyMask)
                else reference.as_bool_key_mask(key_mask))
        if tuple(keys.shape) != (batch, Sk):
            raise ValueError(f"key mask {list(keys.shape)} does not match "
                             f"[batch={batch}, Sk={Sk}]")
        if keys.device != bm.device:
            raise ValueError(f"key mask on {keys.device}, block mask on "
                             f"{bm.device}")
    if bm.is_cuda:
        ext = _require_ext("pack_block_lists")
        if ext is not None:
            if isinstance(key_mask, KeyMask) and key_mask.words is not None:
                words = key_mask.words
            else:
                words = pack_key_mask(
                    keys if keys is not None else
                    torch.ones(batch, Sk, dtype=torch.bool,
                               device=bm.device)).words
            live, nlive = ext.pack_block_lists(bm, words)
            return BlockMask(bm, keys, words, live, nlive, batch, Sq, Sk)
    return BlockMask(bm, keys, batch=batch, Sq=Sq, Sk=Sk)


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


def _block_mask_for(block_mask, key_mask, q, Sq: int, Sk: int) -> BlockMask:
    B = q.shape[0]
    if not isinstance(block_mask, BlockMask):
        if block_mask.device != q.device:
            raise ValueError(f"block mask on {block_mask.device}, q on "
                             f"{q.device}")
        if key_mask is not None:
            key_mask = _key_mask_for(key_mask, q)
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
    if bm.block.device != q.device:
        raise ValueError(f"block mask on {bm.block.device}, q on {q.device}")
    if q.is_cuda and bm.live is None:
        # packed on CPU (or under PA_ALLOW_EAGER) and moved: pack here
        bm = pack_block_mask(bm.block, B, Sq, Sk, bm.keys)
    return bm


def _mask_for(key_mask, block_mask, q, Sq: int, Sk: int):
    """The call's packed mask: None, a KeyMask or a BlockMask (which holds
    the key mask too)."""
    if block_mask is not None:
        return _block_mask_for(block_mask, key_mask, q, Sq, Sk)
    return None if key_mask is None else _key_mask_for(key_mask, q)


def _mask_kw(km) -> dict:
    """``km`` as keyword arguments of reference.attention / ops.attention*."""
    if isinstance(km, BlockMask):
        return {"key_mask": km.keys, "block_mask": km.block}
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


def _attn_native(q, k, v, scale: float, km, bshd: bool,
                 split: Optional[int] = None):
    """One attention call on the native kernels: (output, None), or
    (None, why) when the call is not covered. ``why`` is None when there
    is no extension to ask (PA_ALLOW_EAGER).

    Picks ext.attn_fwd[_bshd][_split][_masked]; ``km`` is None, a KeyMask or
    a BlockMask, whose 3-D ``live`` selects the block-list kernels inside
    the masked entry points. Head dims 64/128 run as they are; other 16-bit
    head dims under 128 are zero-padded up, on the plain BSHD op only (see
    attention_bshd)."""
    name = ("attn_fwd" + ("_bshd" if bshd else "")
            + ("_split" if split is not None else "")
            + ("_masked" if km is not None else ""))
    ext = _require_ext(name)
    if ext is None:
        return None, None
    fn = getattr(ext, name)
    args = (float(scale),)
    if split is not None:
        args += (int(split),)
    if km is not None:
        args += (km.words, km.live, km.nlive)
    D = q.shape[-1]
    if q.dtype in _NATIVE16 and D in (64, 128):
        if not bshd:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        return fn(q, k, v, *args), None
    if q.dtype in _NATIVE16 and D < 128 and bshd and split is None:
        pad = (0, (64 if D <= 64 else 128) - D)
        out = fn(torch.nn.functional.pad(q, pad),
                 torch.nn.functional.pad(k, pad),
                 torch.nn.functional.pad(v, pad), *args)
        return out[..., :D], None
    return None, f"dtype={q.dtype}, D={D}"


def attention(q, k, v, scale: Optional[float] = None,
              key_mask=None, block_mask=None) -> torch.Tensor:
    """Flash-style fused attention, layout [B, H, S, D].

    key_mask: optional KeyMask or raw [B, Sk] bool/integer mask (see
    pack_key_mask for the contract).
    block_mask: optional BlockMask or raw [ceil(Sq/256), ceil(Sk/64)]
    bool/integer mask (see pack_block_mask for the contract). A raw one is
    packed per call, together with key_mask; a packed one already holds its
    key mask, and passing key_mask= beside it raises.

    k and v have q's batch, head count and head dim and one length Sk;
    anything else raises ValueError (nothing is broadcast). B, H or Sq of
    zero returns the empty result, Sk = 0 zeros: no row sees a key."""
    Sq, Sk = _check_qkv(q, k, v, bshd=False)
    scale = _softmax_scale(q, scale)
    km = _mask_for(key_mask, block_mask, q, Sq, Sk)
    if q.is_cuda:
        out, why = _attn_native(q, k, v, scale, km, bshd=False)
        if out is not None:
            return out
        if why is not None:
            _unsupported("attn_fwd", why)
    return reference.attention(q, k, v, scale, **_mask_kw(km))


def attention_bshd(q, k, v, scale: Optional[float] = None,
                   key_mask=None, block_mask=None) -> torch.Tensor:
    """Fused attention on [B, S, H, D] (strided views allowed — e.g. slices
    of a fused qkv projection; no transpose/contiguous copies on GPU).

    Head dims that are not 64/128 but fit under them (SD1.5's 40/80) are
    zero-padded: padding q/k leaves every softmax score unchanged, padded v
    columns are sliced off the output.

    key_mask: optional KeyMask or raw [B, Sk] bool/integer mask (see
    pack_key_mask for the contract). block_mask: optional BlockMask or raw
    [ceil(Sq/256), ceil(Sk/64)] mask, as in attention.

    Cost statement: the pad wastes attention FLOPs
    proportional to Dp/D — 60% at D=40->64, 60% at D=80->128 — plus one
    pad copy of q/k/v per call. This is acceptable because SD1.5 is the
    PLUMBING config (BASELINE config 1 runs it on cpu,cpu); no SD-class
    GPU performance is claimed anywhere. A native D=48/96 tile would need
    fractional per-thread stage vectors (KVBLK*D/8 not divisible by 512
    threads) — not worth the schedule split while no headline depends on
    these shapes.
    """
    Sq, Sk = _check_qkv(q, k, v, bshd=True)
    scale = _softmax_scale(q, scale)
    km = _mask_for(key_mask, block_mask, q, Sq, Sk)
    if q.is_cuda:
        out, why = _attn_native(q, k, v, scale, km, bshd=True)
        if out is not None:
            return out
        if why is not None:
            _unsupported("attn_fwd_bshd", why)
    out = reference.attention(
        q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3),
        scale, **_mask_kw(km),
    )
    return out.permute(0, 2, 1, 3)


def attention_bshd_split(q, k, v, split: int, scale: Optional[float] = None,
                         key_mask=None, block_mask=None):
    """attention_bshd with per-stream outputs: rows [:split] and [split:]
    land in two contiguous tensors (feeds dual-stream projections with no
    reshape copies). key_mask and block_mask as in attention_bshd."""
    Sq, Sk = _check_qkv(q, k, v, bshd=True, split=split)
    scale = _softmax_scale(q, scale)
    km = _mask_for(key_mask, block_mask, q, Sq, Sk)
    if q.is_cuda:
        out, why = _attn_native(q, k, v, scale, km, bshd=True, split=split)
        if out is not None:
            a, b = out
            return a, b
        # 16-bit head dims below 128 still run the native kernel through
        # attention_bshd's zero-pad route (only the split epilogue is
        # composed from slices) — that is no reference-path fallback.
        # Anything else is reported here (unmasked) and by attention_bshd.
        padded = (why is not None and q.dtype in _NATIVE16
                  and q.shape[-1] < 128)
        if km is None and not padded:
            _unsupported("attn_fwd_bshd_split",
                         f"dtype={q.dtype}, D={q.shape[-1]}")
    if isinstance(km, BlockMask):
        out = attention_bshd(q, k, v, scale, block_mask=km)
    else:
        out = attention_bshd(q, k, v, scale, km)
    return out[:, :split].contiguous(), out[:, split:].contiguous()


_NO_BLOCK_LSE = ("block masks are not supported together with the "
                 "log-sum-exp output (attention_lse / attention_bshd_lse take "
                 "key_mask= only)")


def _attn_lse_native(q, k, v, scale: float, km, bshd: bool):
    """_attn_native for the LSE entry points ext.attn_fwd[_bshd]_lse[_masked]:
    ((out, lse), None) or (None, why). The D < 128 zero-pad route is the
    plain BSHD op's: padding q and k leaves every score, so the lse,
    unchanged."""
    name = ("attn_fwd" + ("_bshd" if bshd else "") + "_lse"
            + ("_masked" if km is not None else ""))
    ext = _require_ext(name)
    if ext is None:
        return None, None
    fn = getattr(ext, name)
    args = (float(scale),)
    if km is not None:
        args += (km.words, km.live, km.nlive)
    D = q.shape[-1]
    if q.dtype in _NATIVE16 and D in (64, 128):
        if not bshd:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        return tuple(fn(q, k, v, *args)), None
    if q.dtype in _NATIVE16 and D < 128 and bshd:
        pad = (0, (64 if D <= 64 else 128) - D)
        out, lse = fn(*(torch.nn.functional.pad(t, pad) for t in (q, k, v)),
                      *args)
        return (out[..., :D], lse), None
    return None, f"dtype={q.dtype}, D={D}"


def attention_lse(q, k, v, scale: Optional[float] = None, key_mask=None,
                  block_mask=None):
    """attention that also returns the log-sum-exp: (out [B, H, Sq, D], fp32
    lse [B, H, Sq]), lse = log of the sum over the row's visible keys of
    exp(scale * q.k). Partial results over disjoint key sets combine exactly
    through it (attention_merge).

    Arguments, refusals and empties as in attention; a row that sees no key
    (Sk = 0, a batch element with no live key) has out = 0 and lse = -inf.
    block_mask= raises ValueError: block masks with the lse are not
    supported."""
    if block_mask is not None:
        raise ValueError(f"attention_lse: {_NO_BLOCK_LSE}")
    Sq, Sk = _check_qkv(q, k, v, bshd=False)
    scale = _softmax_scale(q, scale)
    km = _mask_for(key_mask, None, q, Sq, Sk)
    if q.is_cuda:
        res, why = _attn_lse_native(q, k, v, scale, km, bshd=False)
        if res is not None:
            return res
        if why is not None:
            _unsupported("attn_fwd_lse", why)
    return reference.attention(q, k, v, scale, return_lse=True,
                               **_mask_kw(km))


def attention_bshd_lse(q, k, v, scale: Optional[float] = None, key_mask=None,
                       block_mask=None):
    """attention_bshd that also returns the log-sum-exp: (out [B, Sq, H, D],
    fp32 lse [B, Sq, H]); see attention_lse. Strided views and head dims
    under 128 work as in attention_bshd."""
    if block_mask is not None:
        raise ValueError(f"attention_bshd_lse: {_NO_BLOCK_LSE}")
    Sq, Sk = _check_qkv(q, k, v, bshd=True)
    scale = _softmax_scale(q, scale)
    km = _mask_for(key_mask, None, q, Sq, Sk)
    if q.is_cuda:
        res, why = _attn_lse_native(q, k, v, scale, km, bshd=True)
        if res is not None:
            return res
        if why is not None:
            _unsupported("attn_fwd_bshd_lse", why)
    out, lse = reference.attention(
        q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3),
        scale, return_lse=True, **_mask_kw(km))
    return out.permute(0, 2, 1, 3), lse.permute(0, 2, 1).contiguous()


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
