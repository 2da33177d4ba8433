"""Key-padding masks on the reference path (CPU, runs anywhere): op
semantics, the five model families, the engine's batch split and pipeline
mode."""
import pytest
import torch

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models.layers import rope_2d_table
from comfyui_parallelanything_amd.models.registry import MODELS
from comfyui_parallelanything_amd.ops import reference as R
from comfyui_parallelanything_amd.parallel.chain import DeviceChain, make_entry
from comfyui_parallelanything_amd.parallel.engine import ParallelEngine
from comfyui_parallelanything_amd.parallel.pipeline import (
    configure_pipeline,
    pipeline_mode_active,
)


def _differs(a, b):
    """More than ten times apart what the masked comparisons allow."""
    return (a - b).abs().max().item() > 1e-3


def cpu_chain(*pcts):
    return DeviceChain.from_list([make_entry("cpu", p) for p in pcts])


# ---------------------------------------------------------------- op level

SK = 150


def _patterns(sk=SK):
    g = torch.Generator().manual_seed(7)
    right = torch.arange(sk) < 41
    left = torch.arange(sk) >= 70
    hole = ~((torch.arange(sk) >= 30) & (torch.arange(sk) < 131))
    rand = torch.rand(sk, generator=g) < 0.5
    return torch.stack([right, left, hole, rand])


@pytest.fixture(scope="module")
def qkv():
    g = torch.Generator().manual_seed(0)
    B, H, Sq, D = 4, 2, 33, 16
    q = torch.randn(B, H, Sq, D, generator=g)
    k = torch.randn(B, H, SK, D, generator=g)
    v = torch.randn(B, H, SK, D, generator=g)
    return q, k, v


def test_reference_equals_attention_on_gathered_keys(qkv):
    """Masked attention == plain attention over the live keys only, per
    batch element (right-pad, left-pad, hole, random)."""
    q, k, v = qkv
    mask = _patterns()
    out = R.attention(q, k, v, key_mask=mask)
    for b in range(q.shape[0]):
        idx = mask[b].nonzero().flatten()
        ref = R.attention(q[b:b + 1], k[b:b + 1, :, idx], v[b:b + 1, :, idx])
        torch.testing.assert_close(out[b:b + 1], ref, rtol=0, atol=1e-5)


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int32,
                                   torch.int64])
def test_bool_and_integer_masks_agree(qkv, dtype):
    q, k, v = qkv
    mask = _patterns()
    ref = R.attention(q, k, v, key_mask=mask)
    m = mask.to(dtype) * (3 if dtype != torch.bool else 1)  # nonzero = attend
    assert torch.equal(R.attention(q, k, v, key_mask=m), ref)
    assert torch.equal(ops.attention(q, k, v, key_mask=m), ref)


def test_ops_entry_points_follow_the_reference(qkv):
    q, k, v = qkv
    mask = _patterns()
    ref = R.attention(q, k, v, key_mask=mask)
    km = ops.pack_key_mask(mask)
    assert isinstance(km, ops.KeyMask)
    assert km.words is None and km.live is None and km.nlive is None
    assert torch.equal(km.mask, mask)
    qs, ks, vs = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    for key_mask in (mask, km):
        assert torch.equal(ops.attention(q, k, v, key_mask=key_mask), ref)
        out = ops.attention_bshd(qs, ks, vs, key_mask=key_mask)
        assert torch.equal(out.permute(0, 2, 1, 3), ref)
        a, b = ops.attention_bshd_split(qs, ks, vs, 10, key_mask=key_mask)
        assert torch.equal(torch.cat([a, b], 1).permute(0, 2, 1, 3), ref)


def test_all_true_mask_equals_unmasked(qkv):
    q, k, v = qkv
    mask = torch.ones(q.shape[0], SK, dtype=torch.bool)
    torch.testing.assert_close(R.attention(q, k, v, key_mask=mask),
                               R.attention(q, k, v), rtol=0, atol=1e-6)


def test_masked_rows_are_dont_care(qkv):
    """NaN/Inf in masked K/V rows leaves the output unchanged."""
    q, k, v = qkv
    mask = _patterns()
    ref = R.attention(q, k, v, key_mask=mask)
    dead = ~mask[:, None, :, None].expand_as(k)
    kn = torch.where(dead, torch.full_like(k, float("nan")), k)
    vn = torch.where(dead, torch.full_like(v, float("inf")), v)
    out = R.attention(q, kn, vn, key_mask=mask)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref)


def test_empty_batch_element_gives_zeros(qkv):
    q, k, v = qkv
    mask = _patterns().clone()
    mask[1] = False
    out = R.attention(q, k, v, key_mask=mask)
    assert torch.isfinite(out).all()
    assert torch.equal(out[1], torch.zeros_like(out[1]))
    keep = [0, 2, 3]
    ref = R.attention(q[keep], k[keep], v[keep], key_mask=mask[keep])
    assert torch.equal(out[keep], ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16,
                                   torch.float16])
def test_float_masks_raise(qkv, dtype):
    q, k, v = qkv
    m = _patterns().to(dtype)
    with pytest.raises(ValueError, match="additive"):
        ops.pack_key_mask(m)
    with pytest.raises(ValueError, match="additive"):
        R.attention(q, k, v, key_mask=m)
    with pytest.raises(ValueError, match="additive"):
        ops.attention_bshd(*(t.permute(0, 2, 1, 3) for t in (q, k, v)),
                           key_mask=m)


def test_mask_shape_mismatch_raises(qkv):
    q, k, v = qkv
    with pytest.raises(ValueError):
        ops.attention(q, k, v, key_mask=_patterns()[:2])
    with pytest.raises(ValueError):
        R.attention(q, k, v, key_mask=_patterns(SK - 1))


# ------------------------------------------------------------- model level

FAMILIES = ["flux", "sd3", "zimage", "wan", "sd15"]
LENS = [5, 9, 3]          # mixed lengths in one batch
T_PAD = 14                # padded context length


def test_text_positions_do_not_depend_on_context_length():
    """The joint-sequence families give text token i position i and image
    tokens positions that ignore the text length, so truncating the padded
    context is a fair comparison (WAN and the UNet put no positions on the
    context at all)."""
    long = rope_2d_table(4, 4, (4, 6, 6), text_len=T_PAD)
    short = rope_2d_table(4, 4, (4, 6, 6), text_len=max(LENS))
    assert torch.equal(long[:max(LENS)], short[:max(LENS)])
    assert torch.equal(long[T_PAD:], short[max(LENS):])


def _padded_inputs(name, seed=0):
    make, inputs = MODELS[name]
    B = len(LENS)
    x, t, c, kw = inputs(B, tiny=True, dtype=torch.float32)
    g = torch.Generator().manual_seed(100 + seed)
    ctx = torch.randn(B, T_PAD, c.shape[-1], generator=g)
    mask = torch.arange(T_PAD)[None] < torch.tensor(LENS)[:, None]
    garbage = torch.randn(B, T_PAD, c.shape[-1], generator=g) * 100
    ctx = torch.where(mask[..., None], ctx, garbage)
    return x, t, ctx, kw, mask


@pytest.mark.parametrize("name", FAMILIES)
def test_model_output_ignores_masked_padding(name):
    """Garbage-padded context + attention_mask == the context truncated to
    the longest real prompt (mask truncated to match). Without the mask the
    garbage is attended to and the two differ."""
    make, _ = MODELS[name]
    m = make(tiny=True, dtype=torch.float32)
    x, t, ctx, kw, mask = _padded_inputs(name)
    L = max(LENS)
    padded = m(x, t, context=ctx, attention_mask=mask, **kw)
    trunc = m(x, t, context=ctx[:, :L], attention_mask=mask[:, :L], **kw)
    assert torch.isfinite(padded).all()
    # same math on the same live keys; only fp32 summation order differs
    torch.testing.assert_close(padded, trunc, rtol=1e-4, atol=1e-4)
    # integer masks are accepted as they come from a tokenizer
    padded_int = m(x, t, context=ctx, attention_mask=mask.long(), **kw)
    assert torch.equal(padded_int, padded)
    # the mask is what makes them equal
    nomask_padded = m(x, t, context=ctx, **kw)
    nomask_trunc = m(x, t, context=ctx[:, :L], **kw)
    assert _differs(nomask_padded, nomask_trunc)
    assert _differs(nomask_padded, padded)


@pytest.mark.parametrize("name", FAMILIES)
def test_model_float_attention_mask_raises(name):
    make, _ = MODELS[name]
    m = make(tiny=True, dtype=torch.float32)
    x, t, ctx, kw, mask = _padded_inputs(name)
    with pytest.raises(ValueError, match="additive"):
        m(x, t, context=ctx, attention_mask=mask.float(), **kw)


def test_input_builders_add_attention_mask():
    for name, (_, inputs) in MODELS.items():
        x, t, c, kw = inputs(3, tiny=True, dtype=torch.float32)
        assert "attention_mask" not in kw, name
        x2, t2, c2, kw2 = inputs(3, tiny=True, dtype=torch.float32,
                                 text_len=[1, 4, 8])
        # the mask changes nothing else the builder returns
        assert torch.equal(x, x2) and torch.equal(c, c2), name
        am = kw2["attention_mask"]
        assert am.dtype == torch.bool and am.shape == c.shape[:2], name
        assert am.sum(1).tolist() == [1, 4, 8], name
        assert bool(am[1, :4].all()) and not bool(am[1, 4:].any()), name
        _, _, _, kw3 = inputs(3, tiny=True, dtype=torch.float32, text_len=2)
        assert kw3["attention_mask"].sum(1).tolist() == [2, 2, 2], name
        with pytest.raises(ValueError):
            inputs(3, tiny=True, dtype=torch.float32, text_len=[1, 2])
        with pytest.raises(ValueError):
            inputs(3, tiny=True, dtype=torch.float32, text_len=1000)


def test_cli_text_len(capsys):
    from comfyui_parallelanything_amd import cli

    cli.main(["--model", "zimage", "--tiny", "--devices", "cpu", "--batch",
              "2", "--steps", "1", "--dtype", "fp32", "--text-len", "3,6"])
    assert '"text_len": [\n' in capsys.readouterr().out


# ------------------------------------------------------------ engine level

@pytest.mark.parametrize("name", ["flux", "wan"])
def test_engine_split_scatters_the_mask(name):
    """[cpu, cpu] data-parallel over a mixed-length masked batch == the
    single-device result: the [B, T] kwarg is scattered with the batch."""
    make, _ = MODELS[name]
    m = make(tiny=True, dtype=torch.float32)
    x, t, ctx, kw, mask = _padded_inputs(name)
    ref = m(x, t, context=ctx, attention_mask=mask, **kw)
    eng = ParallelEngine(cpu_chain(50, 50), auto_vram_balance=False)
    eng.setup(m)
    out = eng.forward(x, t, context=ctx, attention_mask=mask, **kw)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-5)
    # and the split really carried per-sample masks: another mask, another
    # result
    other = eng.forward(x, t, context=ctx, attention_mask=mask.flip(0), **kw)
    assert _differs(other, ref)


def test_pipeline_mode_carries_the_mask():
    """Batch 1 routes to layer-sharded pipeline mode; the packed mask rides
    to every block as a keyword argument."""
    make, inputs = MODELS["flux"]
    m = make(tiny=True, dtype=torch.float32)
    eng = ParallelEngine(cpu_chain(50, 50), auto_vram_balance=False)
    eng.setup(m, force_copy_lead=True)
    configure_pipeline(eng)
    assert eng.pipeline is not None
    x, t, c, kw = inputs(1, tiny=True, dtype=torch.float32, text_len=[3])
    c = c.clone()
    c[:, 3:] = torch.randn_like(c[:, 3:]) * 100
    ref = m(x, t, context=c, **kw)
    out = eng.forward(x, t, context=c, **kw)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-6)
    assert not pipeline_mode_active()
    unmasked = m(x, t, context=c, y=kw["y"])
    assert _differs(unmasked, ref)
