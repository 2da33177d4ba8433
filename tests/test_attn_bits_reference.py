"""Dense attention masks (attn_mask=) on the CPU: reference.attention against an
explicit fp64 masked softmax, the GPU test's input conditions, the models and
the regional-mask builder against their definitions."""
import itertools

import pytest
import torch

import attn_band_cases as BC
import attn_bits_cases as MC
import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models import layers
from comfyui_parallelanything_amd.models.registry import MODELS
from comfyui_parallelanything_amd.ops import reference as R


@pytest.mark.parametrize("name", list(MC.PATTERNS))
def test_reference_against_dense_fp64(name):
    mask = MC.PATTERNS[name]
    vis = MC.dense(mask)[:, None]
    empty = ~vis.any(-1)[0, 0]
    assert empty[list(MC.EMPTY)].all() == (name == "bernoulli")
    for D, dtype in itertools.product(C.DIMS, C.DTYPES):
        q, k, v = (t.float() for t in MC.qkv(D, dtype))
        ref = BC.dense_softmax_f64(q, k, v, vis)
        # a phantom key would take a quarter of the softmax or more
        s = torch.matmul(q.double(), k.double().transpose(-1, -2)) / D**0.5
        w = 1 / (1 + torch.exp(s.masked_fill(~vis, float("-inf"))).sum(-1))
        assert w[..., ~empty].min() >= 0.25, (D, dtype, w[..., ~empty].min())
        if name == "dontcare":
            k, v = MC.poisoned(k, v)
        out = R.attention(q, k, v, attn_mask=mask)
        C.check(out, ref, *C.TOL_FP32, what=name)
        assert not out[:, :, empty].any() and out[:, :, ~empty].any()
        if (D, dtype) == (64, C.BF16):      # the ops' CPU path, both layouts
            packed = ops.pack_attn_mask(mask, MC.B, MC.SQ, MC.SK)
            assert torch.equal(ops.attention(q, k, v, attn_mask=packed), out)
            a, b = ops.attention_bshd_split(
                *(t.permute(0, 2, 1, 3) for t in (q, k, v)), 100,
                attn_mask=mask[None] if mask.dim() == 2 else mask[:, None])
            assert torch.equal(torch.cat([a, b], 1).permute(0, 2, 1, 3), out)


@pytest.mark.parametrize("name", ["flux", "zimage"])
def test_model_attn_mask_equals_key_padding(name):
    make, inputs = MODELS[name]
    model = make(tiny=True, dtype=torch.float32)
    x, t, ctx, kw = inputs(2, tiny=True, dtype=torch.float32)
    T = ctx.shape[1]
    S = T + (x.shape[2] // 2) * (x.shape[3] // 2)
    pad = torch.arange(T)[None] < torch.tensor([T - 1, max(T // 2, 1)])[:, None]
    keys = torch.cat([pad, torch.ones(2, S - T, dtype=torch.bool)], 1)
    ref = model(x, t, context=ctx, attention_mask=pad, **kw)
    out = model(x, t, context=ctx, attn_mask=keys[:, None, :].expand(2, S, S),
                **kw)
    assert torch.equal(out, ref)
    assert not torch.equal(out, model(x, t, context=ctx, **kw))
    with pytest.raises(ValueError, match="together with attention_mask"):
        model(x, t, context=ctx, attention_mask=pad, attn_mask=keys, **kw)


def test_regional_joint_mask_against_its_definition():
    T, h, w = 7, 3, 4
    maps = [torch.zeros(h, w, dtype=torch.bool) for _ in range(2)]
    maps[0][:, :3] = True
    maps[1][1:, 2:] = True                  # overlaps maps[0] in column 2
    regions = [(0, 3, maps[0]), (2, 6, maps[1])]    # token 2 in both, 6 in none
    mask = layers.regional_joint_mask(T, h, w, regions)
    for i, j in itertools.product(range(T + h * w), repeat=2):
        ti, tj = i < T, j < T
        spans_i = [r for r in regions if ti and r[0] <= i < r[1]]
        spans_j = [r for r in regions if tj and r[0] <= j < r[1]]
        if ti and tj:
            want = any(r[0] <= j < r[1] for r in spans_i)
        elif ti:
            want = any(r[2].reshape(-1)[j - T] for r in spans_i)
        elif tj:
            want = any(r[2].reshape(-1)[i - T] for r in spans_j)
        else:
            want = True
        assert bool(mask[i, j]) == bool(want), (i, j)
    assert not mask[6].any() and not mask[:, 6].any()
