"""gfx950 HIP kernel numerics vs the fp32 torch reference (ops/reference.py).

Every test builds bf16 (or fp32) inputs, runs the native kernel on the GPU,
and compares against the reference computed in fp32 on the SAME inputs.
Run on an MI355X box:  python -m pytest tests -m gpu -x -q
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available(), (
        "native _pa_hip extension must be present on a GPU box"
    )


def _cmp(out, ref, rtol, atol, what=""):
    torch.testing.assert_close(
        out.float().cpu(), ref.float().cpu(), rtol=rtol, atol=atol, msg=what
    )


@pytest.mark.parametrize("shape", [(2, 64, 3072), (1, 7, 128), (4, 1, 3584)])
def test_rms_norm_bf16(shape):
    x = torch.randn(*shape, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(shape[-1], device="cuda", dtype=torch.bfloat16)
    out = ops.rms_norm(x, w)
    ref = R.rms_norm(x.float(), w.float())
    _cmp(out, ref, 2e-2, 2e-2, "rms_norm")


def test_rms_norm_no_weight():
    x = torch.randn(3, 33, 128, device="cuda", dtype=torch.bfloat16)
    out = ops.rms_norm(x, None)
    _cmp(out, R.rms_norm(x.float(), None), 2e-2, 2e-2)


def test_rms_norm_fp32():
    x = torch.randn(5, 257, device="cuda")
    w = torch.randn(257, device="cuda")
    out = ops.rms_norm(x, w)
    _cmp(out, R.rms_norm(x, w), 1e-5, 1e-5)


@pytest.mark.parametrize("B,S,D", [(2, 64, 3072), (3, 17, 64), (1, 4608, 128)])
def test_layer_norm_mod(B, S, D):
    x = torch.randn(B, S, D, device="cuda", dtype=torch.bfloat16)
    sc = torch.randn(B, D, device="cuda", dtype=torch.bfloat16)
    sh = torch.randn(B, D, device="cuda", dtype=torch.bfloat16)
    out = ops.layer_norm_mod(x, sc, sh)
    ref = R.layer_norm_mod(x.float(), sc.float(), sh.float())
    _cmp(out, ref, 2e-2, 5e-2, "layer_norm_mod")


def test_gate_residual():
    r = torch.randn(2, 33, 512, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(2, 512, device="cuda", dtype=torch.bfloat16)
    x = torch.randn(2, 33, 512, device="cuda", dtype=torch.bfloat16)
    out = ops.gate_residual(r, g, x)
    _cmp(out, R.gate_residual(r.float(), g.float(), x.float()), 2e-2, 2e-2)


@pytest.mark.parametrize("B,C,H,W,G", [(2, 320, 32, 32, 32), (1, 64, 8, 8, 8)])
def test_group_norm_silu(B, C, H, W, G):
    x = torch.randn(B, C, H, W, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(C, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(C, device="cuda", dtype=torch.bfloat16)
    out = ops.group_norm_silu(x, G, w, b)
    ref = R.group_norm_silu(x.float(), G, w.float(), b.float())
    _cmp(out, ref, 2e-2, 5e-2, "group_norm_silu")


@pytest.mark.parametrize("B,H,S,D", [(2, 4, 64, 128), (1, 2, 100, 64)])
def test_rope_apply(B, H, S, D):
    x = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    cs = R.rope_freqs(torch.arange(S, device="cuda"), D)
    out = ops.rope_apply(x, cs)
    ref = R.rope_apply(x.float(), cs)
    _cmp(out, ref, 2e-2, 2e-2, "rope_apply")


def test_timestep_embedding():
    t = torch.rand(8, device="cuda")
    out = ops.timestep_embedding(t, 256)
    ref = R.timestep_embedding(t.cpu(), 256)
    _cmp(out, ref, 1e-4, 1e-4, "timestep_embedding")


# ---------------- attention ----------------

@pytest.mark.parametrize(
    "B,H,S,D",
    [
        (1, 1, 64, 64),
        (2, 4, 256, 128),
        (1, 2, 100, 128),   # tail: S % 32 != 0
        (1, 2, 37, 64),     # tail: S < KVBLK boundary cases
        (1, 24, 4608, 128), # FLUX joint-sequence shape
    ],
)
def test_attn_fwd_vs_fp32_reference(B, H, S, D):
    torch.manual_seed(0)
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    out = ops.attention(q, k, v)
    ref = R.attention(q.float(), k.float(), v.float())
    # bf16 P quantization + bf16 output: tolerance ~1e-2 abs
    _cmp(out, ref, 2e-2, 2e-2, f"attn_fwd {B}x{H}x{S}x{D}")


def test_attn_fwd_softmax_scale():
    q = torch.randn(1, 2, 128, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(1, 2, 128, 64, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(1, 2, 128, 64, device="cuda", dtype=torch.bfloat16)
    out = ops.attention(q, k, v, scale=0.25)
    ref = R.attention(q.float(), k.float(), v.float(), scale=0.25)
    _cmp(out, ref, 2e-2, 2e-2)


def test_attn_fwd_outlier_rows():
    """Spiked scores force large rescale steps in the online softmax."""
    torch.manual_seed(1)
    q = torch.randn(1, 1, 256, 128, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(1, 1, 256, 128, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(1, 1, 256, 128, device="cuda", dtype=torch.bfloat16)
    k[0, 0, 200] *= 8.0  # late tile dominates the max
    out = ops.attention(q, k, v)
    ref = R.attention(q.float(), k.float(), v.float())
    _cmp(out, ref, 2e-2, 2e-2, "attn outlier")


def test_attn_fwd_bshd_strided_views():
    """BSHD path on strided fused-qkv views == reference on dense copies."""
    torch.manual_seed(3)
    B, S, H, D = 2, 200, 4, 128
    qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16)
    q, k, v = qkv.unbind(2)  # strided views
    out = ops.attention_bshd(q, k, v)
    ref = R.attention(
        q.permute(0, 2, 1, 3).float(),
        k.permute(0, 2, 1, 3).float(),
        v.permute(0, 2, 1, 3).float(),
    ).permute(0, 2, 1, 3)
    _cmp(out, ref, 2e-2, 2e-2, "attn bshd strided")


def test_attn_fwd_cross_lengths():
    """Sq != Skv (cross-attention, e.g. 77 text tokens)."""
    torch.manual_seed(4)
    q = torch.randn(2, 4, 256, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(2, 4, 77, 64, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(2, 4, 77, 64, device="cuda", dtype=torch.bfloat16)
    out = ops.attention_bshd(
        q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    ).permute(0, 2, 1, 3)
    ref = R.attention(q.float(), k.float(), v.float())
    _cmp(out, ref, 2e-2, 2e-2, "attn cross")


@pytest.mark.parametrize("D", [64, 128])
def test_qk_norm_rope_fused(D):
    """D=64 exercises the lanes>=pairs inactive-lane path (SD3-class heads)."""
    torch.manual_seed(5)
    B, S, H = 2, 100, 4
    qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=torch.bfloat16)
    q, k, v = qkv.unbind(2)
    q_ref = q.clone().permute(0, 2, 1, 3).float()
    k_ref = k.clone().permute(0, 2, 1, 3).float()
    wq = torch.randn(D, device="cuda", dtype=torch.bfloat16)
    wk = torch.randn(D, device="cuda", dtype=torch.bfloat16)
    cs = R.rope_freqs(torch.arange(S, device="cuda"), D)
    ops.qk_norm_rope_(q, k, wq, wk, cs)
    ref_q = R.rope_apply(R.rms_norm(q_ref, wq.float()), cs)
    ref_k = R.rope_apply(R.rms_norm(k_ref, wk.float()), cs)
    _cmp(q.permute(0, 2, 1, 3), ref_q, 3e-2, 3e-2, f"fused qk q D={D}")
    _cmp(k.permute(0, 2, 1, 3), ref_k, 3e-2, 3e-2, f"fused qk k D={D}")


def test_model_forward_gpu_tiny():
    from comfyui_parallelanything_amd.models.registry import flux_inputs, make_flux

    m = make_flux(dev="cuda", dtype=torch.bfloat16, tiny=True)
    x, t, c, kw = flux_inputs(2, dev="cuda", dtype=torch.bfloat16, tiny=True)
    with torch.no_grad():
        out = m(x, t, context=c, **kw)
    assert out.shape == x.shape
    assert torch.isfinite(out.float()).all()


def test_ops_refuse_eager_without_ext(monkeypatch):
    """On a GPU, a missing extension must raise, not silently fall back."""
    import comfyui_parallelanything_amd.ops as O

    monkeypatch.setattr(O, "_EXT", None)
    monkeypatch.setattr(O, "_EXT_TRIED", True)
    monkeypatch.setattr(O, "_ALLOW_EAGER", False)
    x = torch.randn(1, 4, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="Refusing silent eager fallback"):
        O.rms_norm(x, None)


def test_attn_pad_head_dims():
    """SD1.5-style head dims (40/80) via zero-padding == reference."""
    for D in (40, 80):
        torch.manual_seed(D)
        q = torch.randn(1, 3, 128, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn_like(q)
        v = torch.randn_like(q)
        out = ops.attention_bshd(
            q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
        ).permute(0, 2, 1, 3)
        ref = R.attention(q.float(), k.float(), v.float())
        _cmp(out, ref, 2e-2, 2e-2, f"attn pad D={D}")


@pytest.mark.parametrize("D", [64, 128])
def test_pack_joint_qkv_fused(D):
    torch.manual_seed(7)
    B, T, Si, H = 2, 16, 48, 4
    txt_qkv = torch.randn(B, T, 3, H, D, device="cuda", dtype=torch.bfloat16)
    img_qkv = torch.randn(B, Si, 3, H, D, device="cuda", dtype=torch.bfloat16)
    wq_t = torch.randn(D, device="cuda", dtype=torch.bfloat16)
    wk_t = torch.randn(D, device="cuda", dtype=torch.bfloat16)
    wq_i = torch.randn(D, device="cuda", dtype=torch.bfloat16)
    wk_i = torch.randn(D, device="cuda", dtype=torch.bfloat16)
    cs = R.rope_freqs(torch.arange(T + Si, device="cuda"), D)
    q, k, v = ops.pack_joint_qkv(txt_qkv, img_qkv, wq_t, wk_t, wq_i, wk_i, cs)
    # reference composition
    def prep(qkv, wq, wk, cs_slice):
        qq, kk, vv = (t.permute(0, 2, 1, 3).float() for t in qkv.unbind(2))
        qq = R.rope_apply(R.rms_norm(qq, wq.float()), cs_slice)
        kk = R.rope_apply(R.rms_norm(kk, wk.float()), cs_slice)
        return qq, kk, vv
    tq, tk, tv = prep(txt_qkv, wq_t, wk_t, cs[:T])
    iq, ik, iv = prep(img_qkv, wq_i, wk_i, cs[T:])
    ref_q = torch.cat([tq, iq], dim=2).permute(0, 2, 1, 3)
    ref_k = torch.cat([tk, ik], dim=2).permute(0, 2, 1, 3)
    ref_v = torch.cat([tv, iv], dim=2).permute(0, 2, 1, 3)
    _cmp(q, ref_q, 3e-2, 3e-2, "pack q")
    _cmp(k, ref_k, 3e-2, 3e-2, "pack k")
    _cmp(v, ref_v, 0, 0, "pack v")  # bitwise passthrough


def test_gelu_tanh_kernel():
    x = torch.randn(3, 1000, 8, device="cuda", dtype=torch.bfloat16)
    out = ops.gelu_tanh(x)
    ref = torch.nn.functional.gelu(x.float(), approximate="tanh")
    _cmp(out, ref, 2e-2, 2e-2, "gelu")


def test_attn_single_head_batch():
    """B*H == 1 must not take the XCD-decoded grid (regression)."""
    torch.manual_seed(9)
    q = torch.randn(1, 1, 300, 128, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    out = ops.attention(q, k, v)
    ref = R.attention(q.float(), k.float(), v.float())
    _cmp(out, ref, 2e-2, 2e-2, "attn BH=1")


def test_gelu_tanh_strided_slice():
    """gelu on a last-dim slice of a fused projection (no copy path)."""
    proj = torch.randn(2, 64, 21504, device="cuda", dtype=torch.bfloat16)
    mlp = proj[..., 9216:]
    out = ops.gelu_tanh(mlp)
    ref = torch.nn.functional.gelu(mlp.float(), approximate="tanh")
    _cmp(out, ref, 2e-2, 2e-2, "gelu strided")


def test_attn_v3_fallback_env():
    """PA_ATTN_V3=1 once selected the previous-generation kernel. The kernel
    and the option are retired; with the variable set, numerics hold."""
    import os
    import subprocess
    import sys

    code = (
        "import torch;"
        "from comfyui_parallelanything_amd import ops;"
        "from comfyui_parallelanything_amd.ops import reference as R;"
        "torch.manual_seed(0);"
        "q=torch.randn(1,2,256,128,device='cuda',dtype=torch.bfloat16);"
        "k=torch.randn_like(q); v=torch.randn_like(q);"
        "out=ops.attention(q,k,v);"
        "ref=R.attention(q.float(),k.float(),v.float());"
        "import sys;"
        "sys.exit(0 if (out.float()-ref).abs().max().item()<0.05 else 1)"
    )
    env = dict(os.environ, PA_ATTN_V3="1")
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       cwd=os.path.dirname(os.path.dirname(__file__)))
    assert r.returncode == 0


def test_attn_split_outputs():
    torch.manual_seed(11)
    B, S, H, D = 2, 192, 8, 128  # BH=16 (XCD grid) with split mid-sequence
    q = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    a, b = ops.attention_bshd_split(q, k, v, 64)
    full = ops.attention_bshd(q, k, v)
    _cmp(a, full[:, :64], 0, 0, "split txt part")  # same kernel math: bitwise
    _cmp(b, full[:, 64:], 0, 0, "split img part")
    ref = R.attention(
        q.permute(0, 2, 1, 3).float(), k.permute(0, 2, 1, 3).float(),
        v.permute(0, 2, 1, 3).float(),
    ).permute(0, 2, 1, 3)
    _cmp(torch.cat([a, b], dim=1), ref, 2e-2, 2e-2, "split vs reference")


def test_timestep_embed_mlp_fused():
    """Fused sinusoid+Linear+SiLU == composed fp32 reference path."""
    from comfyui_parallelanything_amd.models.layers import MLPEmbedder

    torch.manual_seed(11)
    for K, H in ((256, 3072), (256, 512), (32, 64)):
        emb = MLPEmbedder(K, H).cuda().to(torch.bfloat16)
        t = torch.rand(8, device="cuda")
        out = emb.forward_timestep(t)
        # reference: fp32 sinusoid -> bf16 in_layer -> silu -> out_layer,
        # all in fp32 weights for the comparison target
        sin = R.timestep_embedding(t, K).float()
        h_ref = torch.nn.functional.silu(
            sin @ emb.in_layer.weight.float().t() + emb.in_layer.bias.float()
        )
        ref = h_ref @ emb.out_layer.weight.float().t() + emb.out_layer.bias.float()
        _cmp(out, ref, 3e-2, 3e-2, f"ts_embed_mlp K={K} H={H}")


def test_timestep_embed_mlp_matches_composed_path():
    """GPU fused path ~= the composed kernel path it replaces."""
    from comfyui_parallelanything_amd.models.layers import MLPEmbedder

    torch.manual_seed(12)
    emb = MLPEmbedder(256, 1024).cuda().to(torch.bfloat16)
    t = torch.rand(4, device="cuda")
    fused = emb.forward_timestep(t)
    composed = emb(ops.timestep_embedding(t, 256).to(torch.bfloat16))
    _cmp(fused, composed.float(), 3e-2, 3e-2, "ts mlp fused-vs-composed")


@pytest.mark.parametrize("name", ["flux", "sd15", "zimage", "sd3", "wan_i2v"])
def test_whole_model_gpu_vs_cpu_reference(name):
    """End-to-end composition check: the bf16 HIP-kernel path on GPU vs
    the SAME tiny model in fp32 on CPU (reference ops). Per-op numerics
    tests bound each kernel; this bounds their COMPOSITION through a full
    forward (block stacks, fused qkv/norm/rope paths, MIOpen convs)."""
    import copy

    from comfyui_parallelanything_amd.models.registry import MODELS

    make, inputs = MODELS[name]
    m_ref = make(dev="cpu", dtype=torch.float32, tiny=True)
    # identical weights BY CONSTRUCTION (CPU and CUDA RNGs differ per
    # seed, so re-making on cuda would produce a different init)
    m_gpu = copy.deepcopy(m_ref).to("cuda", torch.bfloat16)
    x, t, c, kw = inputs(2, tiny=True, dtype=torch.float32)
    with torch.no_grad():
        ref = m_ref(x, t, context=c, **kw).float()
        out = m_gpu(
            x.cuda().bfloat16(), t.cuda(),
            context=c.cuda().bfloat16(),
            **{k: (v.cuda().bfloat16() if isinstance(v, torch.Tensor) else v)
               for k, v in kw.items()},
        ).float().cpu()
    # bf16 drift compounds across blocks: bound the relative l2 error and
    # require strong agreement in direction
    rel = (out - ref).norm() / ref.norm()
    assert rel < 0.15, f"{name}: whole-model rel-l2 {rel:.4f}"
    corr = torch.corrcoef(torch.stack([out.flatten(), ref.flatten()]))[0, 1]
    assert corr > 0.99, f"{name}: correlation {corr:.4f}"


# ---------------- small shapes: tails, scalar rungs, gelu exits ----------------

DT16 = pytest.mark.parametrize(
    "dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _qk_ref(qkv_part, w, cs):
    """[B,S,H,D] view -> fp32 rms_norm + rope, back in [B,S,H,D]."""
    x = qkv_part.permute(0, 2, 1, 3).float()
    return R.rope_apply(R.rms_norm(x, w.float()), cs).permute(0, 2, 1, 3)


@DT16
@pytest.mark.parametrize("D", [40, 64, 128])
@pytest.mark.parametrize("B,S,H", [(1, 3, 3), (1, 2, 3), (1, 1, 3)])
def test_qk_norm_rope_row_tails(B, S, H, D, dtype):
    """9, 6 and 3 rows: every residue of the 4-rows-per-wave tail. D=40
    leaves 44 idle lanes that still feed the 64-lane reduction. The v third
    of the fused buffer is not touched."""
    torch.manual_seed(13)
    qkv = torch.randn(B, S, 3, H, D, device="cuda", dtype=dtype)
    before = qkv.clone()
    q, k, v = qkv.unbind(2)
    wq = torch.randn(D, device="cuda", dtype=dtype)
    wk = torch.randn(D, device="cuda", dtype=dtype)
    cs = R.rope_freqs(torch.arange(S, device="cuda"), D)
    ops.qk_norm_rope_(q, k, wq, wk, cs)
    _cmp(q, _qk_ref(before[:, :, 0], wq, cs), 3e-2, 3e-2, "q")
    _cmp(k, _qk_ref(before[:, :, 1], wk, cs), 3e-2, 3e-2, "k")
    assert torch.equal(qkv[:, :, 2], before[:, :, 2]), "v was modified"


@DT16
@pytest.mark.parametrize("D", [40, 128])
@pytest.mark.parametrize("B,T,Si,H", [(1, 2, 3, 3), (1, 1, 1, 1)])
def test_pack_joint_qkv_row_tails(B, T, Si, H, D, dtype):
    torch.manual_seed(14)
    txt = torch.randn(B, T, 3, H, D, device="cuda", dtype=dtype)
    img = torch.randn(B, Si, 3, H, D, device="cuda", dtype=dtype)
    wq_t, wk_t, wq_i, wk_i = (
        torch.randn(D, device="cuda", dtype=dtype) for _ in range(4))
    cs = R.rope_freqs(torch.arange(T + Si, device="cuda"), D)
    q, k, v = ops.pack_joint_qkv(txt, img, wq_t, wk_t, wq_i, wk_i, cs)
    ref_q = torch.cat([_qk_ref(txt[:, :, 0], wq_t, cs[:T]),
                       _qk_ref(img[:, :, 0], wq_i, cs[T:])], dim=1)
    ref_k = torch.cat([_qk_ref(txt[:, :, 1], wk_t, cs[:T]),
                       _qk_ref(img[:, :, 1], wk_i, cs[T:])], dim=1)
    _cmp(q, ref_q, 3e-2, 3e-2, "pack q")
    _cmp(k, ref_k, 3e-2, 3e-2, "pack k")
    assert torch.equal(v, torch.cat([txt[:, :, 2], img[:, :, 2]], dim=1)), \
        "v is not a bitwise passthrough"


@DT16
def test_scalar_rungs_16bit_unaligned_d(dtype):
    """D=20 is no multiple of 8: the 16-bit scalar kernels, not the vector
    ones. Tolerances of the vector-path tests above."""
    torch.manual_seed(15)
    B, S, D = 2, 5, 20
    x = torch.randn(B, S, D, device="cuda", dtype=dtype)
    w = torch.randn(D, device="cuda", dtype=dtype)
    sc = torch.randn(B, D, device="cuda", dtype=dtype)
    sh = torch.randn(B, D, device="cuda", dtype=dtype)
    r = torch.randn(B, S, D, device="cuda", dtype=dtype)
    _cmp(ops.rms_norm(x, w), R.rms_norm(x.float(), w.float()),
         2e-2, 2e-2, "rms_norm")
    _cmp(ops.layer_norm_mod(x, sc, sh),
         R.layer_norm_mod(x.float(), sc.float(), sh.float()),
         2e-2, 5e-2, "layer_norm_mod")
    _cmp(ops.gate_residual(r, sc, x),
         R.gate_residual(r.float(), sc.float(), x.float()),
         2e-2, 2e-2, "gate_residual")


def test_scalar_rungs_fp32():
    """fp32 inputs take the scalar kernels; test_rms_norm_fp32's tolerance."""
    torch.manual_seed(16)
    B, S, D = 2, 5, 24
    x = torch.randn(B, S, D, device="cuda")
    sc = torch.randn(B, D, device="cuda")
    sh = torch.randn(B, D, device="cuda")
    r = torch.randn(B, S, D, device="cuda")
    for out in (ops.layer_norm_mod(x, sc, sh), ops.gate_residual(r, sc, x)):
        assert out.dtype == torch.float32
    _cmp(ops.layer_norm_mod(x, sc, sh), R.layer_norm_mod(x, sc, sh),
         1e-5, 1e-5, "layer_norm_mod fp32")
    _cmp(ops.gate_residual(r, sc, x), R.gate_residual(r, sc, x),
         1e-5, 1e-5, "gate_residual fp32")
    xr = torch.randn(1, 2, 5, 8, device="cuda")
    cs = R.rope_freqs(torch.arange(5, device="cuda"), 8)
    _cmp(ops.rope_apply(xr, cs), R.rope_apply(xr, cs), 1e-5, 1e-5,
         "rope_apply fp32")
    xg = torch.randn(1, 8, 3, 3, device="cuda")
    wg = torch.randn(8, device="cuda")
    bg = torch.randn(8, device="cuda")
    _cmp(ops.group_norm_silu(xg, 4, wg, bg), R.group_norm_silu(xg, 4, wg, bg),
         1e-5, 1e-5, "group_norm_silu fp32")


def test_rms_norm_rejects_float64():
    x = torch.randn(2, 16, device="cuda", dtype=torch.float64)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        ops.rms_norm(x, None)


@DT16
@pytest.mark.parametrize(
    "make",
    [
        lambda dt: torch.randn(24, 16, device="cuda", dtype=dt).t(),  # copy
        lambda dt: torch.randn(4, 6, device="cuda", dtype=dt),   # w % 8 != 0
        lambda dt: torch.randn(3, 5, device="cuda", dtype=dt),   # at::gelu
        lambda dt: torch.randn(16, device="cuda", dtype=dt),     # 1-D
    ],
    ids=["transposed", "w6", "numel15", "1d"],
)
def test_gelu_tanh_exits(make, dtype):
    torch.manual_seed(17)
    x = make(dtype)
    out = ops.gelu_tanh(x)
    assert out.shape == x.shape and out.dtype == dtype
    ref = torch.nn.functional.gelu(x.float(), approximate="tanh")
    _cmp(out, ref, 2e-2, 2e-2, "gelu exits")
