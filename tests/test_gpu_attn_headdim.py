"""Head dims 40 and 80 on their own attention kernels (docs/KERNELS.md,
"Native head dims"): no reference path, the zero-pad route's bits, the fp64
bound of the rounding model, nothing touched at or beyond column D, and
rows off 16 bytes refused.

Sq = 300: two query blocks, the second partial. Sk = 321: five full tiles
and a one-key tail; Sk = 77 (SD cross-attention): one full tile and 13 keys.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A
import kernel_cases as C
from comfyui_parallelanything_amd import ops
from test_gpu_attn_regimes import no_fallback, require_ext  # noqa: F401

B, H = 2, 3
DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DIMS = pytest.mark.parametrize("D", C.PAD_DIMS)
SKS = pytest.mark.parametrize("Sk", [A.SK, 77])
MASK = pytest.mark.parametrize("masked", [False, True],
                               ids=["unmasked", "keys"])


# built once, never modified: CPU case [B, H, S, D], its fp64 reference and
# the three [B, S, H, D] device views
@functools.lru_cache(maxsize=None)
def _case(D, dtype, Sk, masked):
    case = A.rounding_case("peaked", B, H, D, dtype)
    case["k"], case["v"] = case["k"][:, :, :Sk], case["v"][:, :, :Sk]
    if masked:
        # element 0 right-padded (a partial word in the last live tile),
        # element 1 without a live key
        keys = torch.zeros(B, Sk, dtype=torch.bool)
        keys[0, :Sk - 30] = True
        case["keys"] = keys
    bshd = tuple(case[n].cuda().permute(0, 2, 1, 3) for n in "qkv")
    return case, A.reference64(case), bshd


def _keys(case):
    return None if case["keys"] is None else case["keys"].cuda()


@DT
@DIMS
def test_native_path_taken(D, dtype, no_fallback):
    """Neither layout reports the reference path (no_fallback asserts it);
    before these kernels ops.attention did, as ("attn_fwd", "dtype=...,
    D=...")."""
    case, _, (q, k, v) = _case(D, dtype, 77, False)
    assert ops.attention_bshd(q, k, v).shape == (B, A.SQ, H, D)
    q, k, v = (case[n].cuda() for n in "qkv")
    assert ops.attention(q, k, v).shape == (B, H, A.SQ, D)


@MASK
@SKS
@DT
@DIMS
def test_bit_equal_to_pad_route_and_within_bound(D, dtype, Sk, masked,
                                                 no_fallback):
    """The kernel drops only MFMA steps whose operands are all zero from the
    zero-padded run, in the same order: the same bits. And the per-element
    bound of the rounding model against fp64."""
    case, r, (q, k, v) = _case(D, dtype, Sk, masked)
    km, s = _keys(case), 1.0 / math.sqrt(D)
    pad = (0, (64 if D < 64 else 128) - D)
    want = ops.attention_bshd(*(torch.nn.functional.pad(t, pad)
                                for t in (q, k, v)), s, key_mask=km)[..., :D]
    out = ops.attention_bshd(q, k, v, s, key_mask=km)
    assert torch.equal(out, want), (
        f"{(out != want).sum().item()} of {out.numel()} values differ")
    if masked:
        assert torch.equal(out[1], torch.zeros_like(out[1]))
    bhsd = ops.attention(*(case[n].cuda() for n in "qkv"), s, key_mask=km)
    assert torch.equal(bhsd, want.permute(0, 2, 1, 3))
    _, worst = A.model_stats(bhsd, r, dtype)
    print(f"D={D} {dtype} Sk={Sk} masked={masked}: worst |err|/bound "
          f"{worst:.4f}")
    assert worst <= 1.0


@SKS
@DT
@DIMS
def test_nothing_read_past_the_head_dim(D, dtype, Sk, no_fallback):
    """q, k, v are the [..., :D] views of one NaN-filled fused buffer
    [B, S, 3, H, D + 8] (rows beyond Sq / Sk stay NaN too): finite, and the
    bits of the call on exact-size tensors. The op returns a fresh tensor,
    so there is no output view to check."""
    S = max(A.SQ, Sk)
    for masked in (False, True):
        case, _, (q, k, v) = _case(D, dtype, Sk, masked)
        buf = torch.full((B, S, 3, H, D + 8), float("nan"), dtype=dtype,
                         device="cuda")
        buf[:, :A.SQ, 0, :, :D] = q
        buf[:, :Sk, 1, :, :D] = k
        buf[:, :Sk, 2, :, :D] = v
        out = ops.attention_bshd(buf[:, :A.SQ, 0, :, :D], buf[:, :Sk, 1, :, :D],
                                 buf[:, :Sk, 2, :, :D], key_mask=_keys(case))
        assert torch.isfinite(out.float()).all()
        assert torch.equal(out, ops.attention_bshd(q, k, v,
                                                   key_mask=_keys(case)))


@DT
@DIMS
def test_rows_off_16_bytes_are_refused(D, dtype):
    """A head stride of D + 4 elements: every other row starts 8 bytes off.
    Refused by the launcher's own check, and no error is left pending."""
    _, _, (q, k, v) = _case(D, dtype, 77, False)
    buf = torch.zeros(B, A.SQ, H, D + 4, dtype=dtype, device="cuda")
    with pytest.raises(RuntimeError, match="16 bytes"):
        ops.attention_bshd(buf[..., :D], k, v)
    torch.cuda.synchronize()
    assert torch.isfinite(ops.attention_bshd(q, k, v).float()).all()
