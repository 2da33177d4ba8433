"""fp16 as a first-class element type of the gfx950 HIP kernels.

Same structure as test_gpu_kernels.py: fp16 inputs, native kernel on the
GPU, fp32 torch reference (ops/reference.py) on the SAME inputs, and the
tolerances of the matching bf16 tests. On top of that:

- fp16 must be real fp16 (f16 MFMA, RNE f16 packs), not a cast through
  bf16: on values representable in both formats the fp16 kernels must be
  at least 2x closer to the fp32 reference than the bf16 kernels (three
  more mantissa bits predict ~8x).
- an fp16 tensor can never reach a bf16 instantiation: mixed dtypes raise.
- nothing falls back to the eager reference path: after an fp16 forward of
  every model family, ops._WARNED holds no fp16 entry.

Run on an MI355X box:  python -m pytest tests/test_gpu_fp16.py -m gpu -q
"""
import copy
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

F16 = torch.float16
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available(), (
        "native _pa_hip extension must be present on a GPU box"
    )


def _cmp(out, ref, rtol, atol, what=""):
    assert out.dtype == F16, f"{what}: output dtype {out.dtype}"
    torch.testing.assert_close(
        out.float().cpu(), ref.float().cpu(), rtol=rtol, atol=atol, msg=what
    )


def _randn(*shape):
    return torch.randn(*shape, device="cuda", dtype=F16)


def _fp16_fallbacks(keys):
    """Entries of ops._WARNED that name torch.float16 (not torch.bfloat16)."""
    return [k for k in keys if re.search(r"(?<!b)float16", str(k))]


@pytest.fixture()
def no_fallback():
    """Fails the test if an op warned about an fp16 reference-path fallback.

    ops warns once per (op, reason): forget earlier fp16 entries first, so
    a fallback already seen by another test is still caught here."""
    ops._WARNED.difference_update(_fp16_fallbacks(ops._WARNED))
    yield
    fell_back = _fp16_fallbacks(ops._WARNED)
    assert not fell_back, f"fp16 fell back to the reference path: {fell_back}"


def _ref_attn_bhsd(q, k, v, scale=None):
    return R.attention(q.float(), k.float(), v.float(), scale)


# ---------------- direct extension calls ----------------

def test_ext_attn_entry_points_take_fp16():
    ext = ops.hip_ext()
    torch.manual_seed(0)
    q, k, v = (_randn(2, 4, 128, 64) for _ in range(3))
    out = ext.attn_fwd(q, k, v, 0.125)
    assert out.dtype == F16 and out.shape == q.shape
    qs, ks, vs = (_randn(2, 192, 8, 128) for _ in range(3))
    out = ext.attn_fwd_bshd(qs, ks, vs, 0.0884)
    assert out.dtype == F16 and out.shape == qs.shape
    a, b = ext.attn_fwd_bshd_split(qs, ks, vs, 0.0884, 64)
    assert a.dtype == F16 and b.dtype == F16
    assert a.shape == (2, 64, 8, 128) and b.shape == (2, 128, 8, 128)
    assert torch.isfinite(out.float()).all()


# ---------------- attention vs fp32 reference ----------------

@pytest.mark.parametrize(
    "B,H,S,D",
    [
        (1, 1, 64, 64),
        (2, 4, 256, 128),
        (1, 2, 100, 128),   # S % 64 tail
        (1, 2, 37, 64),     # S < one KV tile
        (1, 8, 300, 128),   # BH % 8 == 0: XCD-affine grid, with a tail
        (1, 1, 300, 128),   # BH == 1: 2-D grid
    ],
)
def test_attn_fp16_vs_fp32_reference(B, H, S, D, no_fallback):
    torch.manual_seed(0)
    q, k, v = (_randn(B, H, S, D) for _ in range(3))
    out = ops.attention(q, k, v)
    _cmp(out, _ref_attn_bhsd(q, k, v), 2e-2, 2e-2, f"attn {B}x{H}x{S}x{D}")


def test_attn_fp16_cross_lengths(no_fallback):
    """Sq != Skv (cross-attention, 77 text tokens)."""
    torch.manual_seed(4)
    q = _randn(2, 4, 256, 64)
    k = _randn(2, 4, 77, 64)
    v = _randn(2, 4, 77, 64)
    out = ops.attention_bshd(
        q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    ).permute(0, 2, 1, 3)
    _cmp(out, _ref_attn_bhsd(q, k, v), 2e-2, 2e-2, "attn cross")


def test_attn_fp16_bshd_strided_views(no_fallback):
    torch.manual_seed(3)
    qkv = _randn(2, 200, 3, 4, 128)
    q, k, v = qkv.unbind(2)  # strided views of the fused projection
    out = ops.attention_bshd(q, k, v)
    ref = _ref_attn_bhsd(
        q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    ).permute(0, 2, 1, 3)
    _cmp(out, ref, 2e-2, 2e-2, "attn bshd strided")


@pytest.mark.parametrize("D", [40, 80])
def test_attn_fp16_pad_head_dims(D, no_fallback):
    torch.manual_seed(D)
    q, k, v = (_randn(1, 3, 128, D) for _ in range(3))
    out = ops.attention_bshd(
        q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    ).permute(0, 2, 1, 3)
    _cmp(out, _ref_attn_bhsd(q, k, v), 2e-2, 2e-2, f"attn pad D={D}")


def test_attn_fp16_softmax_scale(no_fallback):
    torch.manual_seed(2)
    q, k, v = (_randn(1, 2, 128, 64) for _ in range(3))
    out = ops.attention(q, k, v, scale=0.25)
    _cmp(out, _ref_attn_bhsd(q, k, v, 0.25), 2e-2, 2e-2, "attn scale")


def test_attn_fp16_outlier_rows(no_fallback):
    """One late key scaled x8 forces a large online-softmax rescale."""
    torch.manual_seed(1)
    q, k, v = (_randn(1, 1, 256, 128) for _ in range(3))
    k[0, 0, 200] *= 8.0
    out = ops.attention(q, k, v)
    _cmp(out, _ref_attn_bhsd(q, k, v), 2e-2, 2e-2, "attn outlier")


def test_attn_fp16_split_outputs(no_fallback):
    torch.manual_seed(11)
    q, k, v = (_randn(2, 192, 8, 128) for _ in range(3))
    a, b = ops.attention_bshd_split(q, k, v, 64)
    full = ops.attention_bshd(q, k, v)
    _cmp(a, full[:, :64], 0, 0, "split txt part")  # same kernel math: bitwise
    _cmp(b, full[:, 64:], 0, 0, "split img part")


# ---------------- bandwidth ops vs fp32 references ----------------

@pytest.mark.parametrize("shape", [(2, 64, 3072), (1, 7, 128), (4, 1, 3584)])
def test_rms_norm_fp16(shape):
    x = _randn(*shape)
    w = _randn(shape[-1])
    _cmp(ops.rms_norm(x, w), R.rms_norm(x.float(), w.float()),
         2e-2, 2e-2, "rms_norm")


def test_rms_norm_fp16_no_weight():
    x = _randn(3, 33, 128)
    _cmp(ops.rms_norm(x, None), R.rms_norm(x.float(), None), 2e-2, 2e-2)


@pytest.mark.parametrize("B,S,D", [(3, 17, 64), (2, 64, 3072)])
def test_layer_norm_mod_fp16(B, S, D):
    x, sc, sh = _randn(B, S, D), _randn(B, D), _randn(B, D)
    ref = R.layer_norm_mod(x.float(), sc.float(), sh.float())
    _cmp(ops.layer_norm_mod(x, sc, sh), ref, 2e-2, 5e-2, "layer_norm_mod")


def test_gate_residual_fp16():
    r, g, x = _randn(2, 33, 512), _randn(2, 512), _randn(2, 33, 512)
    ref = R.gate_residual(r.float(), g.float(), x.float())
    _cmp(ops.gate_residual(r, g, x), ref, 2e-2, 2e-2, "gate_residual")


def test_group_norm_silu_fp16():
    x, w, b = _randn(1, 64, 8, 8), _randn(64), _randn(64)
    ref = R.group_norm_silu(x.float(), 8, w.float(), b.float())
    _cmp(ops.group_norm_silu(x, 8, w, b), ref, 2e-2, 5e-2, "group_norm_silu")


def test_rope_apply_fp16():
    x = _randn(1, 2, 100, 64)
    cs = R.rope_freqs(torch.arange(100, device="cuda"), 64)
    _cmp(ops.rope_apply(x, cs), R.rope_apply(x.float(), cs),
         2e-2, 2e-2, "rope_apply")


def test_gelu_tanh_fp16():
    x = _randn(3, 1000, 8)
    ref = torch.nn.functional.gelu(x.float(), approximate="tanh")
    _cmp(ops.gelu_tanh(x), ref, 2e-2, 2e-2, "gelu")


def test_gelu_tanh_fp16_strided_slice():
    """Last-dim slice of a fused projection: strided-rows path, no copy."""
    proj = _randn(2, 64, 1024)
    mlp = proj[..., 384:]
    ref = torch.nn.functional.gelu(mlp.float(), approximate="tanh")
    _cmp(ops.gelu_tanh(mlp), ref, 2e-2, 2e-2, "gelu strided")


@pytest.mark.parametrize("D", [64, 128])
def test_qk_norm_rope_fp16(D, no_fallback):
    """D=64 exercises the lanes>=pairs inactive-lane path."""
    torch.manual_seed(5)
    B, S, H = 2, 100, 4
    qkv = _randn(B, S, 3, H, D)
    q, k, _ = qkv.unbind(2)  # strided views, rewritten in place
    q_ref = q.clone().permute(0, 2, 1, 3).float()
    k_ref = k.clone().permute(0, 2, 1, 3).float()
    wq, wk = _randn(D), _randn(D)
    cs = R.rope_freqs(torch.arange(S, device="cuda"), D)
    ops.qk_norm_rope_(q, k, wq, wk, cs)
    ref_q = R.rope_apply(R.rms_norm(q_ref, wq.float()), cs)
    ref_k = R.rope_apply(R.rms_norm(k_ref, wk.float()), cs)
    _cmp(q.permute(0, 2, 1, 3), ref_q, 3e-2, 3e-2, f"fused qk q D={D}")
    _cmp(k.permute(0, 2, 1, 3), ref_k, 3e-2, 3e-2, f"fused qk k D={D}")


@pytest.mark.parametrize("D", [64, 128])
def test_pack_joint_qkv_fp16(D, no_fallback):
    torch.manual_seed(7)
    B, T, Si, H = 2, 16, 48, 4
    txt_qkv = _randn(B, T, 3, H, D)
    img_qkv = _randn(B, Si, 3, H, D)
    wq_t, wk_t, wq_i, wk_i = (_randn(D) for _ in range(4))
    cs = R.rope_freqs(torch.arange(T + Si, device="cuda"), D)
    q, k, v = ops.pack_joint_qkv(txt_qkv, img_qkv, wq_t, wk_t, wq_i, wk_i, cs)

    def prep(qkv, wq, wk, cs_slice):
        qq, kk, vv = (t.permute(0, 2, 1, 3).float() for t in qkv.unbind(2))
        qq = R.rope_apply(R.rms_norm(qq, wq.float()), cs_slice)
        kk = R.rope_apply(R.rms_norm(kk, wk.float()), cs_slice)
        return qq, kk, vv

    tq, tk, tv = prep(txt_qkv, wq_t, wk_t, cs[:T])
    iq, ik, iv = prep(img_qkv, wq_i, wk_i, cs[T:])
    _cmp(q, torch.cat([tq, iq], dim=2).permute(0, 2, 1, 3), 3e-2, 3e-2, "pack q")
    _cmp(k, torch.cat([tk, ik], dim=2).permute(0, 2, 1, 3), 3e-2, 3e-2, "pack k")
    _cmp(v, torch.cat([tv, iv], dim=2).permute(0, 2, 1, 3), 0, 0, "pack v")


# ---------------- real fp16, not a cast through bf16 ----------------
#
# Inputs are drawn in fp32 and rounded to bf16; those values are exactly
# representable in fp16 too (up to a negligible subnormal tail), so the
# bf16 and fp16 kernels see the same numbers and share one fp32 reference.
# fp16 has three more mantissa bits than bf16: the predicted error ratio is
# ~1/8 (a CPU emulation of the kernels' rounding points gave 0.12-0.16), a
# path that rounds through bf16 anywhere lands near 1.0. Bound: 0.5.

def _common(*shape):
    """(bf16 tensor, fp16 tensor, fp32 tensor) holding the same values."""
    xb = torch.randn(*shape, device="cuda").to(BF16)
    return xb, xb.to(F16), xb.float()


def _err(out, ref):
    return (out.float() - ref).abs().max().item()


def _assert_fp16_beats_bf16(e16, eb, what):
    print(f"{what}: max_abs_err fp16 {e16:.3e}  bf16 {eb:.3e}  "
          f"ratio {e16 / eb:.3f}")
    assert e16 <= 0.5 * eb, (
        f"{what}: fp16 err {e16:.3e} vs bf16 err {eb:.3e} "
        f"(ratio {e16 / eb:.3f} > 0.5)"
    )


@pytest.mark.parametrize("B,H,S,D",
                         [(1, 2, 100, 128), (2, 4, 256, 64), (1, 2, 37, 64)])
def test_attn_fp16_is_not_bf16_precision(B, H, S, D, no_fallback):
    torch.manual_seed(21)
    (qb, qh, qf), (kb, kh, kf), (vb, vh, vf) = (
        _common(B, H, S, D) for _ in range(3))
    ref = R.attention(qf, kf, vf)
    out16 = ops.attention(qh, kh, vh)
    assert out16.dtype == F16
    _assert_fp16_beats_bf16(_err(out16, ref),
                            _err(ops.attention(qb, kb, vb), ref),
                            f"attention {B}x{H}x{S}x{D}")


@pytest.mark.parametrize("shape", [(2, 64, 3072), (1, 7, 128)])
def test_rms_norm_fp16_is_not_bf16_precision(shape):
    torch.manual_seed(22)
    (xb, xh, xf), (wb, wh, wf) = _common(*shape), _common(shape[-1])
    ref = R.rms_norm(xf, wf)
    out16 = ops.rms_norm(xh, wh)
    assert out16.dtype == F16
    _assert_fp16_beats_bf16(_err(out16, ref), _err(ops.rms_norm(xb, wb), ref),
                            f"rms_norm {shape}")


@pytest.mark.parametrize("B,S,D", [(3, 17, 64), (2, 64, 3072)])
def test_layer_norm_mod_fp16_is_not_bf16_precision(B, S, D):
    torch.manual_seed(23)
    (xb, xh, xf), (cb, ch, cf), (sb, sh, sf) = (
        _common(B, S, D), _common(B, D), _common(B, D))
    ref = R.layer_norm_mod(xf, cf, sf)
    out16 = ops.layer_norm_mod(xh, ch, sh)
    assert out16.dtype == F16
    _assert_fp16_beats_bf16(_err(out16, ref),
                            _err(ops.layer_norm_mod(xb, cb, sb), ref),
                            f"layer_norm_mod {B}x{S}x{D}")


@pytest.mark.parametrize("D", [64, 128])
def test_qk_norm_rope_fp16_is_not_bf16_precision(D, no_fallback):
    torch.manual_seed(24)
    B, S, H = 2, 100, 4
    (qb, qh, qf), (kb, kh, kf) = _common(B, S, H, D), _common(B, S, H, D)
    (wqb, wqh, wqf), (wkb, wkh, wkf) = _common(D), _common(D)
    cs = R.rope_freqs(torch.arange(S, device="cuda"), D)
    ref_q = R.rope_apply(R.rms_norm(qf.permute(0, 2, 1, 3), wqf), cs)
    ref_k = R.rope_apply(R.rms_norm(kf.permute(0, 2, 1, 3), wkf), cs)
    ops.qk_norm_rope_(qh, kh, wqh, wkh, cs)   # in place
    ops.qk_norm_rope_(qb, kb, wqb, wkb, cs)
    assert qh.dtype == F16
    e16 = max(_err(qh.permute(0, 2, 1, 3), ref_q),
              _err(kh.permute(0, 2, 1, 3), ref_k))
    eb = max(_err(qb.permute(0, 2, 1, 3), ref_q),
             _err(kb.permute(0, 2, 1, 3), ref_k))
    _assert_fp16_beats_bf16(e16, eb, f"qk_norm_rope_ D={D}")


# ---------------- no mixing of dtypes ----------------

def test_attn_mixed_dtypes_raise():
    q = _randn(1, 2, 64, 64)
    k = torch.randn(1, 2, 64, 64, device="cuda", dtype=BF16)
    v = _randn(1, 2, 64, 64)
    with pytest.raises(RuntimeError, match="must match"):
        ops.attention(q, k, v)
    with pytest.raises(RuntimeError, match="must match"):
        ops.attention_bshd(q, v, k)


def test_qk_norm_rope_mixed_weight_dtype_raises():
    qkv = _randn(1, 16, 3, 2, 64)
    q, k, _ = qkv.unbind(2)
    before = q.clone()
    w16 = _randn(64)
    wb = torch.randn(64, device="cuda", dtype=BF16)
    cs = R.rope_freqs(torch.arange(16, device="cuda"), 64)
    with pytest.raises(RuntimeError, match="must match"):
        ops.qk_norm_rope_(q, k, wb, w16, cs)
    with pytest.raises(RuntimeError, match="must match"):
        ops.qk_norm_rope_(q, k, w16, wb, cs)
    assert torch.equal(q, before), "q was modified by a rejected call"


# ---------------- whole-model composition ----------------

@pytest.mark.parametrize(
    "name", ["flux", "sd15", "sdxl", "zimage", "sd3", "wan", "wan_i2v"])
def test_whole_model_fp16_gpu_vs_cpu_reference(name):
    """fp16 HIP-kernel path on the GPU vs the SAME tiny model in fp32 on the
    CPU, with the bounds of the bf16 whole-model test, and no fp16 entry in
    ops._WARNED afterwards (nothing fell back to the reference path)."""
    from comfyui_parallelanything_amd.models.registry import MODELS

    make, inputs = MODELS[name]
    m_ref = make(dev="cpu", dtype=torch.float32, tiny=True)
    m_gpu = copy.deepcopy(m_ref).to("cuda", F16)
    x, t, c, kw = inputs(2, tiny=True, dtype=torch.float32)
    ops._WARNED.difference_update(_fp16_fallbacks(ops._WARNED))
    with torch.no_grad():
        ref = m_ref(x, t, context=c, **kw).float()
        out = m_gpu(
            x.cuda().half(), t.cuda(), context=c.cuda().half(),
            **{k: (v.cuda().half() if isinstance(v, torch.Tensor) else v)
               for k, v in kw.items()},
        )
    assert out.dtype == F16
    out = out.float().cpu()
    rel = ((out - ref).norm() / ref.norm()).item()
    corr = torch.corrcoef(
        torch.stack([out.flatten(), ref.flatten()]))[0, 1].item()
    print(f"{name}: fp16 whole-model rel-l2 {rel:.5f} corr {corr:.6f}")
    assert rel < 0.15, f"{name}: whole-model rel-l2 {rel:.4f}"
    assert corr > 0.99, f"{name}: correlation {corr:.4f}"
    fell_back = _fp16_fallbacks(ops._WARNED)
    assert not fell_back, f"{name}: fp16 reference-path fallback {fell_back}"


def test_timestep_mlp_fp16_composed_path():
    """timestep_embed_mlp stays bf16-only; an fp16 MLPEmbedder must take the
    composed path (fp32 sinusoid kernel -> fp16 Linear) and match fp32."""
    from comfyui_parallelanything_amd.models.layers import MLPEmbedder

    torch.manual_seed(12)
    emb = MLPEmbedder(256, 1024).cuda().to(F16)
    t = torch.rand(4, device="cuda")
    out = emb.forward_timestep(t)
    sin = R.timestep_embedding(t, 256).float()
    h_ref = torch.nn.functional.silu(
        sin @ emb.in_layer.weight.float().t() + emb.in_layer.bias.float())
    ref = h_ref @ emb.out_layer.weight.float().t() + emb.out_layer.bias.float()
    _cmp(out, ref, 3e-2, 3e-2, "fp16 timestep MLP (composed)")
