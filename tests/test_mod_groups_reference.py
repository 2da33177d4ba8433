"""Grouped modulation [B, G, D] on the CPU: the reference ops, the refusals
of ops.layer_norm_mod / ops.gate_residual, and per-frame timesteps [B, f]
through the tiny WAN model."""
import pytest
import torch

import kernel_cases as K
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models.wan import WanConfig, WanDiT
from comfyui_parallelanything_amd.ops import reference as R

B, S, D = 2, 12, 24
GROUPS = pytest.mark.parametrize("G", [1, 3, 12])


def _inputs(G, dtype=torch.float32):
    g = torch.Generator().manual_seed(G)
    x, res = 40.0 + torch.randn(2, B, S, D, generator=g)
    mod = torch.randn(3, B, G, D, generator=g)
    return x.to(dtype), res.to(dtype), mod.to(dtype)


@GROUPS
def test_reference_against_fp64(G):
    x, res, (scale, shift, gate) = _inputs(G)
    rows = torch.arange(S) // (S // G)
    ln = K.layer_norm_f64(x) * (1.0 + scale.double()[:, rows]) \
        + shift.double()[:, rows]
    K.check(R.layer_norm_mod(x, scale, shift), ln, *K.TOL_FP32)
    K.check(ops.layer_norm_mod(x, scale, shift), ln, *K.TOL_FP32)
    gr = res.double() + gate.double()[:, rows] * x.double()
    K.check(ops.gate_residual(res, gate, x), gr, *K.TOL_FP32)


@GROUPS
def test_identical_rows_agree_with_2d(G):
    x, res, mod = _inputs(1, torch.bfloat16)
    scale, shift, gate = mod.expand(3, B, G, D)
    assert torch.equal(ops.layer_norm_mod(x, scale, shift),
                       ops.layer_norm_mod(x, mod[0, :, 0], mod[1, :, 0]))
    assert torch.equal(ops.gate_residual(res, gate, x),
                       ops.gate_residual(res, mod[2, :, 0], x))


def _z(*shape, **kw):
    return torch.zeros(*shape, **kw)


# beside x [2, 12, 24] fp32 on the CPU: (error, scale, shift)
REFUSED = {
    "S % G": (ValueError, _z(2, 5, 24), _z(2, 5, 24)),
    "other B": (RuntimeError, _z(3, 3, 24), _z(3, 3, 24)),
    "other D": (RuntimeError, _z(2, 3, 16), _z(2, 3, 16)),
    "dtype": (RuntimeError, _z(2, 3, 24).half(), _z(2, 3, 24).half()),
    "device": (RuntimeError, _z(2, 3, 24, device="meta"),
               _z(2, 3, 24, device="meta")),
    "shapes": (RuntimeError, _z(2, 3, 24), _z(2, 4, 24)),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(name):
    err, scale, shift = REFUSED[name]
    x = _z(B, S, D)
    with pytest.raises(err, match="S = 12.*G = 5" if name == "S % G" else None):
        ops.layer_norm_mod(x, scale, shift)
    if name != "shapes":
        with pytest.raises(err):
            ops.gate_residual(x, scale, x)


def _tiny_wan():
    torch.manual_seed(0)
    model = WanDiT(WanConfig.tiny()).eval()
    # f = 3 frames of 2 x 3 tokens
    return model, torch.randn(2, 4, 3, 4, 6), torch.randn(2, 5, 32)


def test_wan_frame_timesteps():
    """All frames equal is the [B] forward exactly; distinct frames differ
    from it and equal the same forward with every modulation expanded per
    token to [B, S, D], which the reference ops always took."""
    model, x, ctx = _tiny_wan()
    t = torch.tensor([[0.0, 0.5, 0.9], [0.0, 0.2, 0.7]])
    mid = model(x, t[:, 1], context=ctx)
    assert torch.equal(model(x, t[:, 1:2].expand(2, 3), context=ctx), mid)
    out = model(x, t, context=ctx)
    assert not torch.equal(out, mid)

    def per_token(fn, mods):
        def call(*args):
            args = list(args)
            for i in mods:
                assert args[i].shape[1] == 3
                args[i] = args[i].repeat_interleave(args[0].shape[1] // 3, 1)
            return fn(*args)
        return call
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "layer_norm_mod", per_token(R.layer_norm_mod, (1, 2)))
        mp.setattr(ops, "gate_residual", per_token(R.gate_residual, (1,)))
        # the same fp32 operations on the same values: bit for bit
        assert torch.equal(out, model(x, t, context=ctx))


def test_wan_refuses_what_it_cannot_serve():
    model, x, ctx = _tiny_wan()
    for shape in ((3,), (2, 2), (2, 3, 1), ()):
        with pytest.raises(ValueError, match=r"\[B\].*\[B, f\]"):
            model(x, torch.zeros(shape), context=ctx)
    model.transformer_blocks[0].self_qkv.ln_quant = None   # an fp8 Linear's
    with pytest.raises(ValueError, match="layer_norm_mod_fp8"):
        model(x, torch.zeros(2, 3), context=ctx)
    model._seq_parallel = type("SP", (), {"broadcast": lambda s, *a: a})()
    with pytest.raises(ValueError, match="frame edge"):
        model(x, torch.zeros(2, 3), context=ctx)
