"""Row bounds on the CPU against their definitions; the sentinel case's input."""
import copy
import itertools

import pytest
import torch

import attn_band_cases as BC
import kernel_cases as C
from comfyui_parallelanything_amd import ops


@pytest.mark.parametrize("name", list(BC.PATTERNS))
def test_cpu_ops_against_dense_fp64(name):
    lo, hi = BC.PATTERNS[name]
    q, k, v = (t.float() for t in BC.qkv(64, C.BF16))
    ref = BC.dense_softmax_f64(q, k, v, BC.visible(lo, hi))
    empty = lo.clamp(0, BC.SK) >= hi.clamp(0, BC.SK)
    for out in (ops.attention(q, k, v, row_bounds=ops.pack_row_bounds(
                    lo, hi, BC.SQ, BC.SK)),
                ops.attention_bshd(*(t.permute(0, 2, 1, 3) for t in (q, k, v)),
                                   row_bounds=(lo, hi)).permute(0, 2, 1, 3)):
        C.check(out, ref, *C.TOL_FP32, what=name)
        assert not out[:, :, empty].any() and out[:, :, ~empty].any()


def test_sentinel_inputs():
    """A phantom key would take a quarter of the softmax or more, and the
    patterns that catch a -3e30 sentinel have an empty row beside live ones."""
    for name in BC.EMPTY_ROW_PATTERNS:
        seen = BC.visible(*BC.PATTERNS[name])[:256].any(1)
        assert seen.any() and not seen.all(), name
    lo, hi = BC.PATTERNS["sentinel"]
    vis = BC.visible(lo, hi)
    assert not vis[:128, 64:].any() and not vis[128:256, :128].any()
    for D, dtype in itertools.product(C.DIMS, C.DTYPES):
        q, k, _ = BC.qkv(D, dtype)
        s = torch.matmul(q.double(), k.double().transpose(-1, -2)) / D**0.5
        w = 1 / (1 + torch.exp(s.masked_fill(~vis, float("-inf"))).sum(-1))
        assert w[..., :256].min() >= 0.25, (D, dtype, w[..., :256].min())


def test_builders_against_their_definitions():
    for Sq, Sk in ((5, 5), (3, 7), (7, 3)):
        lo, hi = ops.causal_row_bounds(Sq, Sk)
        assert lo.tolist() == [0] * Sq
        assert hi.tolist() == [i + 1 + Sk - Sq for i in range(Sq)]
    for frames, T, back, ahead in ((6, 50, 1, 0), (6, 50, None, 0),
                                   (4, 3, 1, 1), (3, 5, 0, 7)):
        lo, hi = ops.frame_span_row_bounds(frames, T, back, ahead)
        for i in range(frames * T):
            f = i // T
            assert lo[i] == (0 if back is None else max(0, f - back) * T)
            assert hi[i] == min(frames, f + ahead + 1) * T


def test_wan_frame_span_against_dense_mask_softmax(monkeypatch):
    from comfyui_parallelanything_amd.models.wan import WanConfig, WanDiT

    cfg = WanConfig.tiny()
    cfg.self_attn_frame_span = (1, 0)
    torch.manual_seed(0)
    model = WanDiT(cfg).float().eval()
    x, t = torch.randn(1, 4, 4, 6, 10), torch.rand(1)   # f=4, 15 tokens each
    ctx = torch.randn(1, 8, 32)
    out = model(x, t, context=ctx)
    model.cfg = copy.copy(cfg)
    model.cfg.self_attn_frame_span = (None, 3)          # reaches every frame
    dense = model(x, t, context=ctx)
    model.cfg.self_attn_frame_span = None
    assert torch.equal(dense, model(x, t, context=ctx))
    assert len(model._mask_cache) == 1 and (out - dense).abs().max() > 1e-3
    vis = BC.visible(*ops.frame_span_row_bounds(4, 15, 1, 0), Sk=60)
    plain = ops.attention_bshd

    def self_attn_dense(q, k, v, scale=None, **kw):
        if q.shape[1] != k.shape[1]:                    # the cross-attention
            return plain(q, k, v, scale, **kw)
        return BC.dense_softmax_f64(
            *(a.permute(0, 2, 1, 3) for a in (q, k, v)), vis,
            scale).permute(0, 2, 1, 3).float()

    monkeypatch.setattr(ops, "attention_bshd", self_attn_dense)
    C.check(out, model(x, t, context=ctx), 1e-4, 1e-4)

