"""Per-head block masks and the top-p selector on the reference path (no GPU):
the 4-D form of reference.attention, the fp64 selector and the margins that
make its mask a fair yardstick for the kernels, the refusals, the WAN switch.
"""
import copy

import pytest
import torch

import head_block_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

SELECT = pytest.mark.parametrize(
    "name,D,dt", [("small", 64, "bf16"), ("small", 128, "fp16"),
                  ("big", 128, "bf16"), ("big", 64, "fp16")])


def _qkv(B, H, Sq, Sk, D=64, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, H, Sq, D, generator=g),
            torch.randn(B, H, Sk, D, generator=g),
            torch.randn(B, H, Sk, D, generator=g))


@pytest.mark.parametrize("Bm,Hm", [(2, 2), (1, 2), (2, 1), (1, 1)])
def test_per_head_mask_is_each_heads_own_2d_mask(Bm, Hm):
    """Head (b, h) of the 4-D call equals the 2-D call with its own mask on
    that head alone, key mask composed, through ops and a packed mask too; a
    row with no visible key is zero; NaN at keys (b, h) never sees is inert."""
    B, H = 2, 2
    q, k, v = _qkv(B, H, C.SQ, C.SK)
    mask, keys = C.head_mask(B, H)[-Bm:, -Hm:], C.key_mask(B)
    full = mask.expand(B, H, -1, -1)
    out = R.attention(q, k, v, key_mask=keys, block_mask=mask)
    dead = ~C.seen_keys(full, keys)[..., None]
    assert torch.equal(R.attention(q.clone(), k.masked_fill(dead, float("nan")),
                                   v.masked_fill(dead, float("nan")),
                                   key_mask=keys, block_mask=mask.int()), out)
    for b in range(B):
        for h in range(H):
            one = R.attention(q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1],
                              v[b:b + 1, h:h + 1], key_mask=keys[b:b + 1],
                              block_mask=full[b, h])
            torch.testing.assert_close(out[b, h], one[0, 0])
    assert torch.equal(out[1, 1, 512:], torch.zeros(88, 64))
    packed = ops.pack_head_block_mask(mask, B, H, C.SQ, C.SK, key_mask=keys)
    assert (packed.batch, packed.heads, packed.Sq, packed.Sk) == (
        B, H, C.SQ, C.SK)
    got = ops.attention_bshd(*(t.permute(0, 2, 1, 3) for t in (q, k, v)),
                             block_mask=packed)
    assert torch.equal(got.permute(0, 2, 1, 3), out)


def test_refusals_each_followed_by_a_valid_call():
    B, H = 2, 2
    q, k, v = _qkv(B, H, C.SQ, C.SK, seed=2)
    qs, ks, vs = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    mask = C.head_mask(B, H)
    bm = ops.pack_head_block_mask(mask, B, H, C.SQ, C.SK)
    rows = torch.arange(C.SQ)
    for msg, call in (
            ("no split", lambda: ops.attention_bshd_split(
                qs, ks, vs, 100, block_mask=bm)),
            ("lse", lambda: ops.attention_lse(q, k, v, block_mask=bm)),
            ("lse", lambda: ops.attention_bshd_lse(qs, ks, vs,
                                                   block_mask=mask)),
            ("belongs in the pack", lambda: ops.attention(
                q, k, v, key_mask=C.key_mask(B), block_mask=bm)),
            ("row_bounds", lambda: ops.attention(
                q, k, v, block_mask=bm, row_bounds=(rows * 0, rows + 1))),
            ("attn_mask", lambda: ops.attention(
                q, k, v, block_mask=bm,
                attn_mask=torch.ones(C.SQ, C.SK, dtype=torch.bool))),
            ("packed for", lambda: ops.attention(
                q[:, :1], k[:, :1], v[:, :1], block_mask=bm)),
            ("packed for", lambda: ops.attention(
                q[:1, :, :300], k[:1], v[:1], block_mask=bm)),
            ("additive", lambda: ops.attention(
                q, k, v, block_mask=mask.float())),
            ("1 or 2, 1 or 2, 3, 6", lambda: ops.attention(
                q, k, v, block_mask=mask[:, :, :2])),
            ("per-head block mask must be", lambda: ops.pack_head_block_mask(
                mask[0], B, H, C.SQ, C.SK))):
        with pytest.raises(ValueError, match=msg):
            call()
        ops.attention(q, k, v, block_mask=bm)


@SELECT
@pytest.mark.parametrize("top_p", C.TOP_PS[:2])
def test_reference_mask_is_far_from_its_own_boundary(name, D, dt, top_p):
    """What makes torch.equal against this mask a fair check of an fp32
    kernel (pooling and dots of O(1) values err around 1e-5): for every (b,
    h, query block), the kept mass without its lowest tie group is <= top_p -
    1e-3, the kept mass is >= top_p + 1e-3, and the lowest kept score exceeds
    the highest dropped one by >= 1e-3."""
    c = C.select_case(name, D, dt)
    s, p = R.select_scores(c["q"], c["k"])
    sel = R.select_block_mask(c["q"], c["k"], top_p)
    low = s.masked_fill(~sel, float("inf")).amin(-1, keepdim=True)
    without_lowest = (p * (sel & (s > low))).sum(-1)
    assert without_lowest.max() <= top_p - 1e-3
    assert (p * sel).sum(-1).min() >= top_p + 1e-3
    assert (low[..., 0] - s.masked_fill(sel, float("-inf")).amax(-1)
            ).min() >= 1e-3
    if top_p == 0.5:
        # the lowest kept group is the tie pair, and one of the pair alone
        # reaches top_p: a cumulative sum that ignores ties drops the other
        assert ((s == low) & sel).sum(-1).eq(2).all()
        assert (without_lowest + p.masked_fill(s != low, 0).amax(-1)
                ).min() >= top_p


@SELECT
@pytest.mark.parametrize("top_p", C.TOP_PS)
@pytest.mark.parametrize("bshd", [False, True], ids=["bhsd", "bshd"])
def test_ops_select_on_cpu_is_the_reference(name, D, dt, top_p, bshd):
    c = C.select_case(name, D, dt)
    q, k = c["q"], c["k"]
    if bshd:
        q, k = (t.permute(0, 2, 1, 3).contiguous() for t in (q, k))
    got = ops.select_block_mask(q, k, top_p, bshd=bshd, keep=c["keep"])
    assert got.dtype == torch.bool
    assert torch.equal(got, C.select_ref(name, D, dt, top_p))
    assert got.all() == (top_p == 1.0)
    assert c["keep"] is None or got[:, :, c["keep"]].all()


def test_partial_block_and_tile_average_their_real_rows_only():
    """Sq = 600, Sk = 321: the last query block has 88 rows, the last tile
    one key. Their means are over those rows, not over 256 / 64."""
    c = C.select_case("small", 64, "bf16")
    q, k = c["q"].double(), c["k"].double()
    s, _ = R.select_scores(c["q"], c["k"], scale=1.0)
    want = (q[:, :, 512:].mean(2) * k[:, :, 320]).sum(-1)
    torch.testing.assert_close(s[:, :, 2, 5], want)
    want = (q[:, :, :256].mean(2) * k[:, :, 64:128].mean(2)).sum(-1)
    torch.testing.assert_close(s[:, :, 0, 1], want)


def test_select_refusals():
    q, k, _ = _qkv(1, 2, 300, 130)
    for p in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            ops.select_block_mask(q, k, p)
    big = torch.zeros(1, 1, 64 * (ops.SELECT_MAX_TILES + 1), 64)
    with pytest.raises(ValueError, match="cap"):
        ops.select_block_mask(q[:, :1], big, 0.5)
    with pytest.raises(ValueError, match="block mask must be"):
        ops.select_block_mask(q, k, 0.5, keep=torch.ones(2, 2).bool())
    assert ops.select_block_mask(q, k, 0.5).shape == (1, 2, 2, 3)


def test_wan_top_p(capsys):
    """top_p = 1 is the dense forward; 0.5 is not; the frame window's tiles
    are kept; frame spans, sequence parallelism and P outside (0, 1] raise;
    the CLI flag reaches the config and is for WAN only."""
    from comfyui_parallelanything_amd import cli
    from comfyui_parallelanything_amd.models.wan import WanConfig, WanDiT
    from comfyui_parallelanything_amd.parallel import sequence
    from comfyui_parallelanything_amd.parallel.dist import DistInfo

    torch.manual_seed(0)
    model = WanDiT(WanConfig.tiny()).float().eval()
    g = torch.Generator(device="cpu").manual_seed(5)
    args = (torch.randn(2, 4, 6, 16, 16, generator=g),
            torch.rand(2, generator=g))
    ctx = torch.randn(2, 8, 32, generator=g)

    def run(**cfg):
        m = copy.copy(model)
        m.cfg, m._mask_cache = copy.copy(model.cfg), {}
        for key, val in cfg.items():
            setattr(m.cfg, key, val)
        return m(*args, context=ctx)

    dense = run()
    torch.testing.assert_close(run(self_attn_top_p=1.0), dense,
                               rtol=1e-5, atol=1e-5)
    assert (run(self_attn_top_p=0.5) - dense).abs().max() > 1e-3
    assert (run(self_attn_top_p=1e-6)
            - run(self_attn_top_p=1e-6, self_attn_frame_window=0)
            ).abs().max() > 1e-3
    with pytest.raises(ValueError, match="frame_span"):
        run(self_attn_top_p=0.5, self_attn_frame_span=(None, 0))
    with pytest.raises(ValueError, match=r"\(0, 1\]"):
        run(self_attn_top_p=1.5)
    model.cfg.self_attn_top_p = 0.5
    with pytest.raises(ValueError, match="self_attn_top_p"):
        sequence.install_sequence_parallel(
            model, DistInfo(0, 1, 0, torch.device("cpu"), "gloo"))
    cli.main(["--model", "wan", "--tiny", "--attn-top-p", "0.5", "--devices",
              "cpu", "--steps", "1"])
    assert '"attn_top_p": 0.5' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        cli.main(["--model", "flux", "--tiny", "--attn-top-p", "0.5",
                  "--devices", "cpu", "--steps", "1"])
