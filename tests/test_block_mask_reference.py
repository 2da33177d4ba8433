"""Block masks (256 query rows x 64 keys) on the reference path (CPU, runs
anywhere): op semantics, the frame-window pattern, the WAN model and the
CLI."""
import math

import pytest
import torch

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models.wan import WanConfig, WanDiT
from comfyui_parallelanything_amd.ops import reference as R
from comfyui_parallelanything_amd.parallel.chain import DeviceChain, make_entry
from comfyui_parallelanything_amd.parallel.engine import ParallelEngine
from comfyui_parallelanything_amd.parallel.pipeline import _move

# the project's fp32 figure (tests/test_models.py)
RTOL = ATOL = 1e-5


# ---------------------------------------------------------------- op level

B, H, SQ, SK, D = 2, 2, 600, 321, 16      # nq = 3, nk = 6 (last tile 1 key)


@pytest.fixture(scope="module")
def qkv():
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, H, SQ, D, generator=g)
    k = torch.randn(B, H, SK, D, generator=g)
    v = torch.randn(B, H, SK, D, generator=g)
    return q, k, v


def _block():
    """Query block 0 sees tiles 0 and 3, block 1 nothing, block 2 tiles 2,
    4 and the one-key tile 5. Tile 1 is seen by nobody."""
    m = torch.zeros(3, 6, dtype=torch.bool)
    m[0, 0] = m[0, 3] = True
    m[2, 2] = m[2, 4] = m[2, 5] = True
    return m


def _keys():
    g = torch.Generator().manual_seed(3)
    keys = torch.rand(B, SK, generator=g) < 0.6
    keys[1, 128:192] = False    # element 1: tile 2 has no live key
    return keys


def _visible(block, keys=None):
    """[B, Sq, Sk] visibility from the definition, one entry at a time
    (index arithmetic, no repeat_interleave)."""
    i = torch.arange(SQ)[:, None] // 256
    j = torch.arange(SK)[None, :] // 64
    vis = block[i, j][None].expand(B, SQ, SK)
    if keys is not None:
        vis = vis & keys[:, None, :]
    return vis


def _dense_softmax(q, k, v, vis):
    """Independent dense-mask attention: explicit exp / sum, invisible
    terms multiplied out instead of pushed to -inf."""
    vis = vis[:, None]                                   # [B, 1, Sq, Sk]
    s = torch.einsum("bhid,bhjd->bhij", q, k) / math.sqrt(q.shape[-1])
    top = torch.where(vis, s, torch.full((), -1e30)).amax(-1, keepdim=True)
    # (a row with nothing visible: every term is multiplied out, sum 0)
    e = torch.exp((s - top).clamp(max=0.0)) * vis
    p = e / e.sum(-1, keepdim=True).clamp(min=1e-30)
    return torch.einsum("bhij,bhjd->bhid", p, v)


@pytest.mark.parametrize("with_keys", [False, True], ids=["block", "block+keys"])
def test_reference_equals_dense_mask_softmax(qkv, with_keys):
    q, k, v = qkv
    block, keys = _block(), (_keys() if with_keys else None)
    out = R.attention(q, k, v, key_mask=keys, block_mask=block)
    torch.testing.assert_close(out, _dense_softmax(q, k, v, _visible(block, keys)),
                               rtol=RTOL, atol=ATOL)
    # the empty query block gives exact zeros, its neighbours do not
    assert torch.equal(out[:, :, 256:512], torch.zeros(B, H, 256, D))
    assert out[:, :, :256].abs().min(dim=-1).values.max() > 0
    assert out[:, :, 512:].abs().amax(-1).min() > 0
    # through the public op, raw and packed
    torch.testing.assert_close(
        ops.attention(q, k, v, key_mask=keys, block_mask=block.long()), out,
        rtol=0, atol=0)
    bm = ops.pack_block_mask(block, B, SQ, SK, key_mask=keys)
    assert bm.words is None and bm.live is None and bm.nlive is None
    assert torch.equal(bm.block, block)
    torch.testing.assert_close(ops.attention(q, k, v, block_mask=bm), out,
                               rtol=0, atol=0)
    qs, ks, vs = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    torch.testing.assert_close(
        ops.attention_bshd(qs, ks, vs, block_mask=bm).permute(0, 2, 1, 3),
        out, rtol=0, atol=0)
    lo, hi = ops.attention_bshd_split(qs, ks, vs, 100, block_mask=bm)
    torch.testing.assert_close(torch.cat([lo, hi], 1).permute(0, 2, 1, 3),
                               out, rtol=0, atol=0)


def test_all_true_block_mask_is_dense_attention(qkv):
    q, k, v = qkv
    out = R.attention(q, k, v, block_mask=torch.ones(3, 6, dtype=torch.int32))
    torch.testing.assert_close(out, R.attention(q, k, v), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("with_keys", [False, True], ids=["block", "block+keys"])
def test_never_visible_keys_are_dont_care(qkv, with_keys):
    """NaN in K/V at keys no query row of the batch element sees: tile 1
    for everybody, and with the key mask its dead keys and element 1's
    whole tile 2."""
    q, k, v = qkv
    block, keys = _block(), (_keys() if with_keys else None)
    unseen = ~_visible(block, keys).any(dim=1)           # [B, Sk]
    assert unseen[:, 64:128].all() and not unseen.all()
    if with_keys:
        assert unseen[1, 128:192].all() and not unseen[0, 128:192].all()
    rows = unseen[:, None, :, None].expand_as(k)
    out = R.attention(q, k.masked_fill(rows, float("nan")),
                      v.masked_fill(rows, float("nan")),
                      key_mask=keys, block_mask=block)
    assert torch.isfinite(out).all()
    assert torch.equal(out, R.attention(q, k, v, key_mask=keys,
                                        block_mask=block))


def test_float_and_misshaped_block_masks_raise(qkv):
    q, k, v = qkv
    for call in (lambda m: R.attention(q, k, v, block_mask=m),
                 lambda m: ops.attention(q, k, v, block_mask=m),
                 lambda m: ops.pack_block_mask(m, B, SQ, SK)):
        with pytest.raises(ValueError, match="additive"):
            call(_block().float())
        with pytest.raises(ValueError, match=r"\[3, 6\]"):
            call(torch.ones(3, 5, dtype=torch.bool))
        with pytest.raises(ValueError, match=r"\[3, 6\]"):
            call(torch.ones(2, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="key mask"):
        ops.pack_block_mask(_block(), B, SQ, SK, key_mask=_keys()[:1])


def test_packed_block_mask_refuses_a_separate_key_mask(qkv):
    q, k, v = qkv
    bm = ops.pack_block_mask(_block(), B, SQ, SK)
    qs, ks, vs = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    with pytest.raises(ValueError, match="belongs in the pack"):
        ops.attention(q, k, v, key_mask=_keys(), block_mask=bm)
    with pytest.raises(ValueError, match="belongs in the pack"):
        ops.attention_bshd(qs, ks, vs, key_mask=_keys(), block_mask=bm)
    with pytest.raises(ValueError, match="belongs in the pack"):
        ops.attention_bshd_split(qs, ks, vs, 10, key_mask=_keys(),
                                 block_mask=bm)


def test_block_mask_packed_for_another_problem_raises(qkv):
    q, k, v = qkv
    for other in ((B + 1, SQ, SK), (B, SQ - 256, SK), (B, SQ, SK - 64)):
        nq, nk = R.block_mask_shape(other[1], other[2])
        bm = ops.pack_block_mask(torch.ones(nq, nk, dtype=torch.bool), *other)
        with pytest.raises(ValueError, match="packed for"):
            ops.attention(q, k, v, block_mask=bm)


def test_geometry_constants_and_pipeline_move():
    assert ops.ATTN_Q_BLOCK == 256 and ops.ATTN_KV_TILE == 64
    bm = ops.pack_block_mask(_block(), B, SQ, SK, key_mask=_keys())
    moved = _move(bm, torch.device("cpu"))
    assert isinstance(moved, ops.BlockMask)
    assert torch.equal(moved.block, bm.block) and torch.equal(moved.keys, bm.keys)
    assert (moved.batch, moved.Sq, moved.Sk) == (B, SQ, SK)


# ------------------------------------------------------- frame-window mask

def test_frame_window_small_case():
    m = ops.frame_window_block_mask(3, 100, 0)
    assert m.dtype == torch.bool
    assert m.int().tolist() == [[1, 1, 1, 1, 1], [0, 0, 0, 1, 1]]


@pytest.mark.parametrize("window,density", [(0, 0.0513), (1, 0.1416),
                                            (2, 0.2275), (4, 0.3857)])
def test_frame_window_wan_720p(window, density):
    m = ops.frame_window_block_mask(21, 3600, window)
    assert tuple(m.shape) == (296, 1182)
    assert abs(m.float().mean().item() - density) <= 1e-4
    if window == 0:
        assert m.sum(dim=1).min().item() >= 57


def test_frame_window_matches_the_definition_entry_by_entry():
    frames, T, window = 5, 150, 1
    S = frames * T
    m = ops.frame_window_block_mask(frames, T, window)
    for i in range(m.shape[0]):
        qlo, qhi = (256 * i) // T, (min(256 * (i + 1), S) - 1) // T
        for t in range(m.shape[1]):
            klo, khi = (64 * t) // T, (min(64 * (t + 1), S) - 1) // T
            assert bool(m[i, t]) == (khi >= qlo - window and klo <= qhi + window)


def test_frame_window_covering_every_frame_is_all_true():
    for frames, window in ((21, 20), (21, 25), (1, 0)):
        assert ops.frame_window_block_mask(frames, 3600, window).all()
    with pytest.raises(ValueError):
        ops.frame_window_block_mask(4, 64, -1)


# ------------------------------------------------------------------- model

def _wan(window=None):
    cfg = WanConfig.tiny()
    cfg.self_attn_frame_window = window
    torch.manual_seed(0)
    return WanDiT(cfg).float().eval()


@pytest.fixture(scope="module")
def video():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 4, 6, 16, 16, generator=g)    # f=6, T=64, S=384
    t = torch.rand(2, generator=g)
    ctx = torch.randn(2, 8, 32, generator=g)
    return x, t, ctx


def test_wan_frame_window_zero_is_two_independent_clips(video):
    """window=0 at f=6, T=64: query block 0 (rows 0-255) sees exactly frames
    0-3 and block 1 exactly frames 4-5, and RoPE enters attention only
    through position differences, so the masked forward equals the dense
    forward of each clip alone. Bound: rtol = atol = 1e-4, the issue's
    starting figure; it holds here as it stands."""
    x, t, ctx = video
    block = ops.frame_window_block_mask(6, 64, 0)
    assert block.int().tolist() == [[1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 1, 1]]
    out = _wan(0)(x, t, context=ctx)
    dense = _wan()
    head = dense(x[:, :, :4].contiguous(), t, context=ctx)
    tail = dense(x[:, :, 4:].contiguous(), t, context=ctx)
    for name, got, want in (("frames 0-3", out[:, :, :4], head),
                            ("frames 4-5", out[:, :, 4:], tail)):
        print(f"{name}: max abs err {(got - want).abs().max().item():.3e}")
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    # and a leak would show: the dense forward of all six frames is far off
    assert (dense(x, t, context=ctx) - out).abs().max() > 1e-2


def test_wan_window_reaching_every_frame_is_the_dense_forward(video):
    x, t, ctx = video
    ref = _wan()(x, t, context=ctx)
    m = _wan(5)
    assert torch.equal(m(x, t, context=ctx), ref)
    assert not m._mask_cache, "window >= f - 1 must not build a mask"
    assert not torch.equal(_wan(0)(x, t, context=ctx), ref)


def test_wan_mask_cache_is_keyed_on_the_batch_size(video):
    x, t, ctx = video
    m = _wan(0)
    both = m(x, t, context=ctx)
    one = m(x[:1], t[:1], context=ctx[:1])
    assert len(m._mask_cache) == 2
    assert sorted(bm.batch for bm in m._mask_cache.values()) == [1, 2]
    torch.testing.assert_close(one, both[:1], rtol=1e-4, atol=1e-5)
    m(x, t, context=ctx)
    assert len(m._mask_cache) == 2


def test_engine_split_packs_per_replica(video):
    """[cpu, cpu] data-parallel: each replica packs for its own chunk."""
    x, t, ctx = video
    m = _wan(0)
    ref = m(x, t, context=ctx)
    eng = ParallelEngine(
        DeviceChain.from_list([make_entry("cpu", 50), make_entry("cpu", 50)]),
        auto_vram_balance=False)
    eng.setup(m)
    out = eng.forward(x, t, context=ctx)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-5)


# --------------------------------------------------------------------- CLI

def test_cli_frame_window(capsys):
    from comfyui_parallelanything_amd import cli

    cli.main(["--model", "wan", "--tiny", "--frame-window", "1", "--devices",
              "cpu", "--steps", "1"])
    assert '"frame_window": 1' in capsys.readouterr().out


def test_cli_frame_window_is_for_wan_only():
    from comfyui_parallelanything_amd import cli

    with pytest.raises(SystemExit) as err:
        cli.main(["--model", "flux", "--tiny", "--frame-window", "1",
                  "--devices", "cpu", "--steps", "1"])
    assert err.value.code not in (0, None)
