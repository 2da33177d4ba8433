"""Per-head block masks and the top-p selector on the native gfx950 kernels.

Attention: against ops.reference.attention in fp32 on the CPU under the same
4-D mask, kernel_cases.check (rtol = atol = 2e-2) on negative_scores inputs,
where a wrong tile moves the output by far more. Selector: torch.equal with
the fp64 reference's mask, which test_head_block_mask_reference.py shows to be
1e-3 from its own boundary, a hundred times the kernels' fp32 error.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import head_block_cases as H_
import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

DTYPES = pytest.mark.parametrize("dt", ["bf16", "fp16"])
DIMS = pytest.mark.parametrize("D", [64, 128])
SQ, SK = H_.SQ, H_.SK


@pytest.fixture(autouse=True)
def native_only(monkeypatch):
    """Skips without a GPU; fails if any call took the reference path."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available("pack_head_block_lists")
    assert ops.hip_available("select_block_mask")
    seen = []
    monkeypatch.setattr(ops, "_unsupported",
                        lambda op, why: seen.append((op, why)))
    yield
    assert not seen, f"fell back to the reference path: {seen}"


def _case(B, H, D, dt, seed=50):
    q, k, v = C.negative_scores(B, H, SQ, SK, D, H_.DTYPES[dt], seed)
    return q.cuda(), k.cuda(), v.cuda()


def _ref(q, k, v, mask, keys=None):
    return R.attention(q.float().cpu(), k.float().cpu(), v.float().cpu(),
                       key_mask=None if keys is None else keys.cpu(),
                       block_mask=mask.cpu())


@pytest.mark.parametrize("H", [2, 4])  # B*H = 4: 2-D grid; 8: XCD 1-D grid
@DTYPES
@DIMS
def test_per_head_lists(D, dt, H):
    """(a) a different pattern for every (b, h), one tile killed for the last
    batch element by the key mask, against the reference; (b) the empty list
    gives exact zeros; (c) NaN in K/V of head h at the tiles (b, h) never
    visits changes no bit: lists indexed by b alone would read it; (d) the
    same pattern for all (b, h) gives the bits of the 2-D call, and Bm = 1 /
    Hm = 1 the bits of the expanded mask."""
    B = 2
    q, k, v = _case(B, H, D, dt)
    mask, keys = H_.head_mask(B, H).cuda(), H_.key_mask(B).cuda()
    out = ops.attention(q, k, v, key_mask=keys, block_mask=mask)
    C.check(out, _ref(q, k, v, mask, keys), what="per-head mask")
    assert torch.equal(out[1, H - 1, 512:], torch.zeros_like(out[0, 0, 512:]))
    assert out[0, 0, 512:].float().abs().amax(-1).min() > 0
    seen = H_.seen_keys(mask, keys)
    assert not seen.all(-1).any(), "every (b, h) leaves some tile unvisited"
    kn = k.masked_fill(~seen[..., None], float("nan"))
    vn = v.masked_fill(~seen[..., None], float("nan"))
    bm = ops.pack_head_block_mask(mask, B, H, SQ, SK, key_mask=keys)
    got = ops.attention_bshd(q.permute(0, 2, 1, 3), kn.permute(0, 2, 1, 3),
                             vn.permute(0, 2, 1, 3), block_mask=bm)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got.permute(0, 2, 1, 3), out)
    shared = mask[0, 0]
    want = ops.attention(q, k, v, block_mask=shared)
    for m4 in (shared[None, None], shared.expand(B, H, -1, -1)):
        assert torch.equal(ops.attention(q, k, v, block_mask=m4), want)
    for m4 in (mask[:1], mask[:, :1], mask[:1, :1].long()):
        full = m4.expand(B, H, -1, -1).contiguous()
        assert torch.equal(ops.attention(q, k, v, block_mask=m4),
                           ops.attention(q, k, v, block_mask=full))


@pytest.mark.parametrize("Sk", [SK, 4480])  # 70 tiles: 2 compaction steps
@pytest.mark.parametrize("Bm,Hm", [(3, 2), (1, 2), (3, 1)])
def test_pack_outputs(Bm, Hm, Sk):
    """(e) live, nlive and the zero tails equal a torch computation."""
    B, H = 3, 2
    nq, nk = R.block_mask_shape(SQ, Sk)
    g = torch.Generator(device="cpu").manual_seed(Sk + Bm)
    mask = torch.rand(Bm, Hm, nq, nk, generator=g) < 0.6
    mask[0, 0, -1] = False
    keys = torch.rand(B, Sk, generator=g) < 0.5
    keys &= ~(torch.rand(B, nk, generator=g) < 0.4).repeat_interleave(
        64, 1)[:, :Sk]
    bm = ops.pack_head_block_mask(mask.cuda().to(torch.uint8) * 3, B, H, SQ,
                                  Sk, key_mask=keys.cuda())
    tile_live = torch.nn.functional.pad(
        keys, (0, nk * 64 - Sk)).view(B, nk, 64).any(-1)
    alive = mask.expand(B, H, -1, -1) & tile_live[:, None, None, :]
    order = torch.argsort((~alive).int(), dim=-1, stable=True)
    live = torch.where(torch.arange(nk) < alive.sum(-1, keepdim=True), order,
                       torch.zeros((), dtype=torch.long))
    assert bm.live.dtype == bm.nlive.dtype == torch.int32
    assert torch.equal(bm.words, ops.pack_key_mask(keys.cuda()).words)
    assert torch.equal(bm.nlive.cpu(), alive.sum(-1).int())
    assert torch.equal(bm.live.cpu(), live.int())


def test_launcher_refusals_each_followed_by_a_valid_call():
    """(f) what only the GPU path can refuse; the ops' own refusals are in
    test_head_block_mask_reference.py."""
    B, H = 2, 2
    q, k, v = _case(B, H, 64, "bf16", seed=52)
    qs, ks, vs = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    mask = H_.head_mask(B, H).cuda()
    bm = ops.pack_head_block_mask(mask, B, H, SQ, SK)
    ext = ops.hip_ext()
    other_h = ops.pack_head_block_mask(mask[:, :1], B, 1, SQ, SK)
    other_sq = ops.pack_head_block_mask(mask[:, :, :2], B, H, 300, SK)
    ref = _ref(q, k, v, mask)
    for exc, msg, call in (
            (ValueError, "no split", lambda: ops.attention_bshd_split(
                qs, ks, vs, 100, block_mask=bm)),
            (ValueError, "packed for", lambda: ops.attention(
                q, k, v, block_mask=other_h)),
            (RuntimeError, "no split", lambda: ext.attn_fwd_bshd_split_masked(
                qs, ks, vs, 0.125, 100, bm.words, bm.live, bm.nlive)),
            (RuntimeError, "log-sum-exp", lambda: ext.attn_fwd_lse_masked(
                q, k, v, 0.125, bm.words, bm.live, bm.nlive)),
            (RuntimeError, "head count", lambda: ext.attn_fwd_masked(
                q, k, v, 0.125, bm.words, other_h.live, other_h.nlive)),
            (RuntimeError, "another Sq", lambda: ext.attn_fwd_masked(
                q, k, v, 0.125, bm.words, other_sq.live, other_sq.nlive)),
            (RuntimeError, r"1 or \(B, H\)", lambda: ext.pack_head_block_lists(
                mask, bm.words, 3)),
            (ValueError, "bf16 or fp16", lambda: ops.select_block_mask(
                q.float(), k.float(), 0.5)),
            (RuntimeError, "16 bytes", lambda: ops.select_block_mask(
                torch.nn.functional.pad(q, (4, 0))[..., 4:], k, 0.5))):
        with pytest.raises(exc, match=msg):
            call()
        C.check(ops.attention(q, k, v, block_mask=bm), ref)


@pytest.mark.parametrize("bshd", [False, True], ids=["bhsd", "bshd"])
@pytest.mark.parametrize("top_p", H_.TOP_PS)
@pytest.mark.parametrize("name,D,dt", [
    ("small", 64, "bf16"), ("small", 64, "fp16"), ("small", 128, "bf16"),
    ("small", 128, "fp16"), ("big", 64, "fp16"), ("big", 128, "bf16")])
def test_select_equals_the_fp64_reference(name, D, dt, top_p, bshd):
    """big: Sk = 19 200, every per-thread tile loop takes a second trip, and
    a keep mask. bshd: views of a wider buffer, strides of their own."""
    c = H_.select_case(name, D, dt)
    q, k = c["q"].cuda(), c["k"].cuda()
    if bshd:
        q, k = (torch.cat([t.permute(0, 2, 1, 3), t.permute(0, 2, 1, 3)],
                          -1)[..., :D] for t in (q, k))
    keep = None if c["keep"] is None else c["keep"].cuda()
    got = ops.select_block_mask(q, k, top_p, bshd=bshd, keep=keep)
    assert got.dtype == torch.bool and got.is_cuda
    assert torch.equal(got.cpu(), H_.select_ref(name, D, dt, top_p))


@DTYPES
@DIMS
def test_select_pack_attend_and_graph_replay(D, dt):
    """select -> pack -> attention equals reference.attention under the
    reference's mask; the same chain captured in one graph follows new q / k
    copied into its static buffers: nothing is read on the host."""
    c = H_.select_case("small", D, dt)
    B, H = c["q"].shape[:2]
    g = torch.Generator(device="cpu").manual_seed(53)
    v = torch.randn(c["k"].shape, generator=g).to(c["k"].dtype).cuda()

    def chain(q, k):
        sel = ops.select_block_mask(q, k, 0.5)
        return ops.attention(
            q, k, v, block_mask=ops.pack_head_block_mask(sel, B, H, SQ, SK))

    q_a, k_a = c["q"].cuda(), c["k"].cuda()
    # the same ladders with the heads exchanged: another mask
    q_b, k_b = q_a.flip(1).contiguous(), k_a.flip(1).contiguous()
    mask_a = H_.select_ref("small", D, dt, 0.5)
    assert not torch.equal(mask_a, mask_a.flip(1))
    sq, sk = q_a.clone(), k_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(sq, sk)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = chain(sq, sk)
    for q_, k_, m_ in ((q_a, k_a, mask_a), (q_b, k_b, mask_a.flip(1)),
                       (q_a, k_a, mask_a)):
        sq.copy_(q_)
        sk.copy_(k_)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, chain(q_, k_))
        C.check(static_out, _ref(q_, k_, v, m_), what="graph replay")


def test_wan_top_p_gpu_vs_cpu_reference():
    """WanDiT.tiny() with self_attn_top_p = 0.5: bf16 native kernels against
    the same weights in fp32 on the CPU reference path, at
    test_wan_frame_window_gpu_vs_cpu_reference's bound."""
    from comfyui_parallelanything_amd.models.wan import WanConfig, WanDiT

    cfg = WanConfig.tiny()
    cfg.self_attn_top_p = 0.5
    torch.manual_seed(0)
    m_ref = WanDiT(cfg).float().eval()
    m_gpu = copy.deepcopy(m_ref).to("cuda", torch.bfloat16)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(2, 4, 6, 16, 16, generator=g)
    t = torch.rand(2, generator=g)
    c = torch.randn(2, 8, 32, generator=g)
    with torch.no_grad():
        ref = m_ref(x, t, context=c).float()
        out = m_gpu(x.cuda().bfloat16(), t.cuda(),
                    context=c.cuda().bfloat16()).float().cpu()
    rel = (out - ref).norm() / ref.norm()
    assert rel < 0.15, f"whole-model rel-l2 {rel:.4f}"
    corr = torch.corrcoef(torch.stack([out.flatten(), ref.flatten()]))[0, 1]
    assert corr > 0.99, f"correlation {corr:.4f}"
