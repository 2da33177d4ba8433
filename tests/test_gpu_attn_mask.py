"""Key-padding masks on the native gfx950 attention kernels.

Reference for every numerics check: ops.reference.attention on fp32 copies
with the same mask, at the tolerances the unmasked attention tests use
(test_gpu_kernels.py for bf16, test_gpu_fp16.py for fp16: rtol = atol = 2e-2).
"""
import copy
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

BF16 = torch.bfloat16
F16 = torch.float16
RTOL = ATOL = 2e-2


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available("attn_fwd_bshd_masked"), (
        "native _pa_hip extension with the masked kernels must be present"
    )


@pytest.fixture()
def no_fallback(monkeypatch):
    """Fails the test if any attention call took the reference path."""
    seen = []
    orig = ops._unsupported

    def spy(op, why):
        seen.append((op, why))
        return orig(op, why)

    monkeypatch.setattr(ops, "_unsupported", spy)
    yield seen
    attn = [s for s in seen if s[0].startswith("attn_fwd")]
    assert not attn, f"attention fell back to the reference path: {attn}"


def _cmp(out, ref, what=""):
    torch.testing.assert_close(out.float().cpu(), ref.float().cpu(),
                               rtol=RTOL, atol=ATOL, msg=what)


def _randn(*shape, dtype=BF16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to("cuda", dtype)


def _ref(q, k, v, mask, scale=None):
    """fp32 reference on [B, H, S, D]."""
    return R.attention(q.float(), k.float(), v.float(), scale, key_mask=mask)


def _ref_bshd(q, k, v, mask, scale=None):
    return _ref(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                v.permute(0, 2, 1, 3), mask, scale).permute(0, 2, 1, 3)


def _ar(sk):
    return torch.arange(sk, device="cuda")


def right_pad(sk):
    """Live [0, L), L inside a tile."""
    return _ar(sk) < sk - 20


def left_pad(sk):
    """At least 64 dead keys first, so tile 0 is dead. At Sk=64 that leaves
    no live key: the zeros-for-empty rule is what the reference gives."""
    return _ar(sk) >= (70 if sk > 70 else 64)


def hole(sk):
    """Dead [L, T): the joint txt|img layout with padded text. Partial tiles
    at both ends, whole dead tiles between them once Sk allows (200, 320)."""
    return ~((_ar(sk) >= 30) & (_ar(sk) < max(sk - 30, 34)))


def bernoulli(sk):
    g = torch.Generator(device="cpu").manual_seed(sk)
    return (torch.rand(sk, generator=g) < 0.5).cuda()


def one_in_last_tile(sk):
    """Exactly one live key in the last tile (the last key); with more than
    one tile, a few live keys in tile 0 too."""
    m = torch.zeros(sk, dtype=torch.bool, device="cuda")
    m[sk - 1] = True
    if sk > 64:
        m[:10] = True
    return m


def all_true(sk):
    return torch.ones(sk, dtype=torch.bool, device="cuda")


GROUPS = [(right_pad, left_pad, hole), (bernoulli, one_in_last_tile, all_true)]


# ---------------- shape and pattern sweep ----------------

@pytest.mark.parametrize("Sk", [64, 100, 200, 320])
@pytest.mark.parametrize("Sq", [37, 300])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_masked_attention_sweep(D, dtype, Sq, Sk, no_fallback):
    B, H = 3, 2  # one batch element per mask pattern, three per call
    q = _randn(B, H, Sq, D, dtype=dtype, seed=1)
    k = _randn(B, H, Sk, D, dtype=dtype, seed=2)
    v = _randn(B, H, Sk, D, dtype=dtype, seed=3)
    for group in GROUPS:
        mask = torch.stack([p(Sk) for p in group])
        out = ops.attention(q, k, v, key_mask=mask)
        assert out.dtype == dtype and out.shape == q.shape
        ref = _ref(q, k, v, mask)
        for b, p in enumerate(group):
            _cmp(out[b], ref[b], f"{p.__name__} D={D} Sq={Sq} Sk={Sk}")
        if all_true in group:
            b = group.index(all_true)
            _cmp(out[b], ops.attention(q, k, v)[b], "all-true vs unmasked op")


# ---------------- contract ----------------

@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_masked_rows_are_dont_care(D, dtype, no_fallback):
    """NaN in every masked K/V row — rows of dead tiles and masked rows of
    partly live tiles — must not reach the output: it equals the run with
    those rows zeroed, bit for bit. Fails if a dead tile is processed or a
    masked row reaches an MFMA."""
    B, H, Sq, Sk = 3, 2, 300, 200
    mask = torch.stack([p(Sk) for p in GROUPS[0]])  # right, left, hole
    q = _randn(B, H, Sq, D, dtype=dtype, seed=4)
    k = _randn(B, H, Sk, D, dtype=dtype, seed=5)
    v = _randn(B, H, Sk, D, dtype=dtype, seed=6)
    dead = ~mask[:, None, :, None].expand_as(k)
    out_zero = ops.attention(q, k.masked_fill(dead, 0.0),
                             v.masked_fill(dead, 0.0), key_mask=mask)
    out_nan = ops.attention(q, k.masked_fill(dead, float("nan")),
                            v.masked_fill(dead, float("nan")), key_mask=mask)
    assert torch.isfinite(out_nan.float()).all()
    assert torch.equal(out_nan, out_zero)
    _cmp(out_nan, _ref(q, k, v, mask), "don't-care rows vs reference")


@pytest.mark.parametrize("D", [64, 128])
def test_empty_batch_element_gives_zeros(D, no_fallback):
    """nlive == 0 next to normal elements: zeros for it, the others are
    right, and the call returns."""
    B, H, Sq, Sk = 3, 2, 300, 200
    mask = torch.stack([right_pad(Sk), torch.zeros_like(all_true(Sk)),
                        bernoulli(Sk)])
    q = _randn(B, H, Sq, D, seed=7)
    # the empty element's K/V are don't-care as well
    k = _randn(B, H, Sk, D, seed=8)
    v = _randn(B, H, Sk, D, seed=9)
    k[1] = float("nan")
    v[1] = float("nan")
    out = ops.attention(q, k, v, key_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(out[1], torch.zeros_like(out[1]))
    ref = _ref(q, k, v, mask)
    _cmp(out[0], ref[0], "element before the empty one")
    _cmp(out[2], ref[2], "element after the empty one")


@pytest.mark.parametrize("tiles", [(0, 2), (1,)], ids=["live02", "live1"])
@pytest.mark.parametrize("D", [64, 128])
def test_odd_pipeline_depths(D, tiles, no_fallback):
    """Sk=192: the D=128 one-barrier pipeline's prologue and prefetch at
    nlive = 2 (with a dead tile between) and nlive = 1 (dead tiles around)."""
    B, H, Sq, Sk = 2, 2, 300, 192
    m = torch.zeros(Sk, dtype=torch.bool, device="cuda")
    for t in tiles:
        m[64 * t:64 * (t + 1)] = True
    mask = torch.stack([m, m])
    q = _randn(B, H, Sq, D, seed=10)
    k = _randn(B, H, Sk, D, seed=11)
    v = _randn(B, H, Sk, D, seed=12)
    dead = ~mask[:, None, :, None].expand_as(k)
    out = ops.attention(q, k.masked_fill(dead, float("nan")),
                        v.masked_fill(dead, float("nan")), key_mask=mask)
    km = ops.pack_key_mask(mask)
    assert km.nlive.tolist() == [len(tiles)] * B
    assert km.live[0, :len(tiles)].tolist() == list(tiles)
    _cmp(out, _ref(q, k, v, mask), f"live tiles {tiles}")


# ---------------- call routes ----------------

@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_masked_bshd_strided_views(dtype, no_fallback):
    B, S, H, D = 3, 200, 4, 128
    qkv = _randn(B, S, 3, H, D, dtype=dtype, seed=13)
    q, k, v = qkv.unbind(2)  # strided views of a fused projection
    mask = torch.stack([p(S) for p in GROUPS[0]])
    out = ops.attention_bshd(q, k, v, key_mask=mask)
    _cmp(out, _ref_bshd(q, k, v, mask), "masked bshd strided")


@pytest.mark.parametrize("D", [64, 128])
def test_masked_cross_lengths(D, no_fallback):
    """Sq=256 against 77 padded text tokens; a packed KeyMask serves several
    calls."""
    B, H = 2, 4
    q = _randn(B, 256, H, D, seed=14)
    k = _randn(B, 77, H, D, seed=15)
    v = _randn(B, 77, H, D, seed=16)
    mask = torch.stack([_ar(77) < 9, _ar(77) < 70])
    km = ops.pack_key_mask(mask)
    ref = _ref_bshd(q, k, v, mask)
    _cmp(ops.attention_bshd(q, k, v, key_mask=km), ref, "cross, packed")
    _cmp(ops.attention_bshd(q, k, v, key_mask=mask.long()), ref,
         "cross, raw int64 mask")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_masked_split_outputs(dtype, no_fallback):
    B, S, H, D = 2, 192, 8, 128  # BH=16: XCD grid, split mid-sequence
    q = _randn(B, S, H, D, dtype=dtype, seed=17)
    k = _randn(B, S, H, D, dtype=dtype, seed=18)
    v = _randn(B, S, H, D, dtype=dtype, seed=19)
    # txt|img joint layout: 64 text slots, 20 / 50 real tokens
    mask = torch.stack([(_ar(S) < 20) | (_ar(S) >= 64),
                        (_ar(S) < 50) | (_ar(S) >= 64)])
    a, b = ops.attention_bshd_split(q, k, v, 64, key_mask=mask)
    assert a.shape == (B, 64, H, D) and b.shape == (B, S - 64, H, D)
    assert a.is_contiguous() and b.is_contiguous()
    full = ops.attention_bshd(q, k, v, key_mask=mask)
    assert torch.equal(a, full[:, :64])  # same kernel math: bitwise
    assert torch.equal(b, full[:, 64:])
    _cmp(torch.cat([a, b], 1), _ref_bshd(q, k, v, mask), "masked split")


@pytest.mark.parametrize("D", [40, 80])
def test_masked_pad_head_dims(D, no_fallback):
    B, S, H = 2, 150, 4
    q = _randn(B, S, H, D, seed=20)
    k = _randn(B, 77, H, D, seed=21)
    v = _randn(B, 77, H, D, seed=22)
    mask = torch.stack([_ar(77) < 12, _ar(77) >= 66])
    out = ops.attention_bshd(q, k, v, key_mask=mask)
    assert out.shape == q.shape
    _cmp(out, _ref_bshd(q, k, v, mask), f"masked pad route D={D}")
    a, b = ops.attention_bshd_split(q, k, v, 50, key_mask=mask)
    assert torch.equal(torch.cat([a, b], 1), out)


def test_fp32_gpu_masked_takes_reference_path():
    """fp32 has no native instantiation: reference path, mask honoured."""
    q = _randn(2, 2, 40, 64, dtype=torch.float32, seed=23)
    k = _randn(2, 2, 90, 64, dtype=torch.float32, seed=24)
    v = _randn(2, 2, 90, 64, dtype=torch.float32, seed=25)
    mask = torch.stack([_ar(90) < 5, _ar(90) >= 64])
    out = ops.attention(q, k, v, key_mask=mask)
    torch.testing.assert_close(out, _ref(q, k, v, mask), rtol=0, atol=1e-5)


# ---------------- pack_key_mask ----------------

def _pack_on_cpu(mask):
    m = mask.cpu().ne(0)
    B, Sk = m.shape
    nt = (Sk + 63) // 64
    words = torch.zeros(B, nt, dtype=torch.int64)
    live = torch.zeros(B, nt, dtype=torch.int32)
    nlive = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        n = 0
        for t in range(nt):
            w = 0
            for j, bit in enumerate(m[b, 64 * t:64 * (t + 1)].tolist()):
                w |= int(bit) << j
            if w >= 1 << 63:
                w -= 1 << 64  # two's complement into int64
            words[b, t] = w
            if w != 0:
                live[b, n] = t
                n += 1
        nlive[b] = n
    return words, live, nlive


@pytest.mark.parametrize("Sk", [1, 64, 100, 200, 320, 64 * 70 + 5])
@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int32,
                                   torch.int64])
def test_pack_key_mask_outputs(Sk, dtype):
    """Words, live list (zero-filled tail) and count equal a CPU
    computation; Sk = 64*70+5 needs a second 64-tile compaction step."""
    g = torch.Generator(device="cpu").manual_seed(Sk)
    rows = [p(Sk).cpu() for p in (right_pad, left_pad, hole, bernoulli,
                                  one_in_last_tile, all_true)]
    rows.append(torch.zeros(Sk, dtype=torch.bool))
    # whole dead tiles scattered among live ones
    tiles = torch.rand((Sk + 63) // 64, generator=g) < 0.5
    rows.append(tiles.repeat_interleave(64)[:Sk])
    mask = torch.stack(rows)
    if dtype != torch.bool:
        mask = mask.to(dtype) * 5  # nonzero = attend
    km = ops.pack_key_mask(mask.cuda())
    words, live, nlive = _pack_on_cpu(mask)
    assert km.words.dtype == torch.int64 and km.live.dtype == torch.int32
    assert km.nlive.dtype == torch.int32 and km.mask.dtype == torch.bool
    assert torch.equal(km.words.cpu(), words)
    assert torch.equal(km.nlive.cpu(), nlive)
    assert torch.equal(km.live.cpu(), live)
    assert torch.equal(km.mask.cpu(), mask.ne(0))


def test_float_mask_raises_on_gpu():
    m = all_true(64).float()[None]
    with pytest.raises(ValueError, match="additive"):
        ops.pack_key_mask(m)
    with pytest.raises(RuntimeError, match="additive"):
        ops.hip_ext().pack_key_mask(m)


def test_launcher_rejects_mismatched_masks():
    ext = ops.hip_ext()
    q = _randn(2, 100, 2, 64, seed=26)
    k = _randn(2, 100, 2, 64, seed=27)
    km = ops.pack_key_mask(torch.stack([all_true(100)] * 2))
    args = (q, k, k, 0.125)
    ext.attn_fwd_bshd_masked(*args, km.words, km.live, km.nlive)
    with pytest.raises(RuntimeError, match="another Sk"):
        other = ops.pack_key_mask(torch.stack([all_true(200)] * 2))
        ext.attn_fwd_bshd_masked(*args, other.words, other.live, other.nlive)
    with pytest.raises(RuntimeError, match="batch"):
        three = ops.pack_key_mask(torch.stack([all_true(100)] * 3))
        ext.attn_fwd_bshd_masked(*args, three.words, three.live, three.nlive)
    with pytest.raises(RuntimeError, match="int64 words"):
        ext.attn_fwd_bshd_masked(*args, km.words.int(), km.live, km.nlive)
    with pytest.raises(RuntimeError, match="device"):
        ext.attn_fwd_bshd_masked(*args, km.words.cpu(), km.live, km.nlive)
    with pytest.raises(ValueError, match="batch"):
        ops.attention_bshd(q, k, k, key_mask=torch.stack([all_true(100)] * 3))


def test_retired_v3_env_never_gives_a_wrong_result():
    """PA_ATTN_V3=1 once selected a bf16-only kernel without masks, which
    had to refuse fp16 and masked calls. The kernel and the option are
    retired: with the variable set, an fp16 call, a masked call and a masked
    split call (last 20 of 64 keys dead) match the fp32 reference at this
    file's tolerance. Child process: the variable was read once per
    process."""
    code = (
        "import torch\n"
        "from comfyui_parallelanything_amd import ops\n"
        "from comfyui_parallelanything_amd.ops import reference as R\n"
        "torch.manual_seed(31)\n"
        "def ref(q, k, v, m=None):\n"
        "    p = lambda t: t.permute(0, 2, 1, 3).float()\n"
        "    return R.attention(p(q), p(k), p(v), None,"
        " key_mask=m).permute(0, 2, 1, 3)\n"
        "def close(out, want, dtype):\n"
        "    assert out.dtype == dtype, out.dtype\n"
        f"    torch.testing.assert_close(out.float(), want,"
        f" rtol={RTOL}, atol={ATOL})\n"
        "h = [torch.randn(1, 64, 2, 64, device='cuda', dtype=torch.float16)\n"
        "     for _ in range(3)]\n"
        "close(ops.attention_bshd(*h), ref(*h), torch.float16)\n"
        "b = [torch.randn(1, 64, 2, 64, device='cuda', dtype=torch.bfloat16)\n"
        "     for _ in range(3)]\n"
        "m = (torch.arange(64, device='cuda') < 44)[None]\n"
        "want = ref(*b, m)\n"
        "assert (want - ref(*b)).abs().max() > 1e-2, 'mask masks nothing'\n"
        "close(ops.attention_bshd(*b, key_mask=m), want, torch.bfloat16)\n"
        "lo, hi = ops.attention_bshd_split(*b, 16, key_mask=m)\n"
        "assert lo.shape[1] == 16 and hi.shape[1] == 48\n"
        "close(torch.cat([lo, hi], dim=1), want, torch.bfloat16)\n"
        "assert not ops._WARNED, ops._WARNED\n"
    )
    env = dict(os.environ, PA_ATTN_V3="1")
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       cwd=os.path.dirname(os.path.dirname(__file__)))
    assert r.returncode == 0


# ---------------- graph replay ----------------

def test_masked_attention_graph_replay(no_fallback):
    """Capture pack + masked attention; replay after copying another mask
    into the static buffer: the result follows the new mask (no host-side
    length or allocation was baked in)."""
    B, S, H, D = 2, 200, 4, 128
    q = _randn(B, S, H, D, seed=28)
    k = _randn(B, S, H, D, seed=29)
    v = _randn(B, S, H, D, seed=30)
    mask_a = torch.stack([right_pad(S), hole(S)])
    mask_b = torch.stack([left_pad(S), one_in_last_tile(S)])
    static_mask = mask_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention_bshd(q, k, v, key_mask=static_mask)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = ops.attention_bshd(q, k, v, key_mask=static_mask)
    graph.replay()
    _cmp(static_out, _ref_bshd(q, k, v, mask_a), "replay, captured mask")
    static_mask.copy_(mask_b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out,
                       ops.attention_bshd(q, k, v, key_mask=mask_b))
    _cmp(static_out, _ref_bshd(q, k, v, mask_b), "replay, new mask")


# ---------------- whole models ----------------

@pytest.mark.parametrize("name", ["flux", "sd3", "zimage", "wan_i2v", "sd15"])
def test_whole_model_masked_gpu_vs_cpu_reference(name, no_fallback):
    """One tiny model per family with a mixed-length attention_mask: bf16
    native kernels on GPU vs the same weights in fp32 on the CPU reference
    path, at test_whole_model_gpu_vs_cpu_reference's bound. The padded
    context tokens are garbage on both sides."""
    from comfyui_parallelanything_amd.models.registry import MODELS

    make, inputs = MODELS[name]
    m_ref = make(dev="cpu", dtype=torch.float32, tiny=True)
    m_gpu = copy.deepcopy(m_ref).to("cuda", torch.bfloat16)
    x, t, c, kw = inputs(2, tiny=True, dtype=torch.float32, text_len=[3, 6])
    am = kw["attention_mask"]
    c = torch.where(am[..., None], c, c * 30)
    with torch.no_grad():
        ref = m_ref(x, t, context=c, **kw).float()
        unmasked = m_ref(x, t, context=c,
                         **{k: v for k, v in kw.items()
                            if k != "attention_mask"}).float()
        out = m_gpu(
            x.cuda().bfloat16(), t.cuda(), context=c.cuda().bfloat16(),
            **{k: (v.cuda().bfloat16() if v.is_floating_point() else v.cuda())
               for k, v in kw.items()},
        ).float().cpu()
    assert (unmasked - ref).abs().max() > 1e-3, "mask had no effect"
    rel = (out - ref).norm() / ref.norm()
    assert rel < 0.15, f"{name}: whole-model rel-l2 {rel:.4f}"
    corr = torch.corrcoef(torch.stack([out.flatten(), ref.flatten()]))[0, 1]
    assert corr > 0.99, f"{name}: correlation {corr:.4f}"


def test_fp8_mode_masked_forward_keeps_fused_paths(monkeypatch, no_fallback):
    """The fp8 serving mode does not touch attention: a masked forward still
    goes through the fused LN+quant path and stays finite."""
    from comfyui_parallelanything_amd.models.quant import (
        FP8Linear, _supports_scaled_mm, quantize_fp8,
    )
    from comfyui_parallelanything_amd.models.registry import (
        flux_inputs, make_flux,
    )

    if not _supports_scaled_mm() or not ops.hip_available("layer_norm_mod_fp8"):
        pytest.skip("no fp8 fused-LN path")
    m = make_flux(dev="cuda", dtype=BF16, tiny=True)
    quantize_fp8(m, min_features=32)
    calls = {"n": 0}
    orig = FP8Linear.ln_quant

    def spy(self, *a, **k):
        calls["n"] += 1
        return orig(self, *a, **k)

    monkeypatch.setattr(FP8Linear, "ln_quant", spy)
    x, t, c, kw = flux_inputs(2, dev="cuda", dtype=BF16, tiny=True,
                              text_len=[3, 6])
    with torch.no_grad():
        out = m(x, t, context=c, **kw)
    assert torch.isfinite(out.float()).all()
    assert calls["n"] > 0, "fused LN+quant path not taken"


def test_engine_hip_graph_follows_the_mask(no_fallback):
    """The engine's graph runner keys and copies the [B, T] kwarg like any
    tensor kwarg: after capture, a replay with another mask gives that
    mask's result."""
    from comfyui_parallelanything_amd.models.registry import (
        make_zimage, zimage_inputs,
    )
    from comfyui_parallelanything_amd.parallel.chain import (
        DeviceChain, make_entry,
    )
    from comfyui_parallelanything_amd.parallel.engine import ParallelEngine

    m = make_zimage(dev="cuda:0", dtype=BF16, tiny=True)
    x, t, c, kw_a = zimage_inputs(2, dev="cuda:0", dtype=BF16, tiny=True,
                                  text_len=[2, 7])
    kw_b = dict(kw_a, attention_mask=kw_a["attention_mask"].flip(0))
    with torch.no_grad():
        ref_a = m(x, t, context=c, **kw_a).clone()
        ref_b = m(x, t, context=c, **kw_b).clone()
    assert (ref_a.float() - ref_b.float()).abs().max() > 1e-2
    eng = ParallelEngine(
        DeviceChain.from_list([make_entry("cuda:0", 100)]),
        auto_vram_balance=False, use_hip_graphs=True,
    )
    eng.setup(m)
    for i in range(4):  # two eager warmups, capture, replay
        out = eng.forward(x, t, context=c, **kw_a)
        torch.cuda.synchronize()
        torch.testing.assert_close(out, ref_a, rtol=2e-2, atol=2e-2)
    assert eng.graphs._graphs, "no hipGraph was captured after warmup"
    out = eng.forward(x, t, context=c, **kw_b)
    torch.cuda.synchronize()
    torch.testing.assert_close(out, ref_b, rtol=2e-2, atol=2e-2)
    assert len(eng.graphs._graphs) == 1, "the mask's values re-keyed the graph"
    eng.release()
