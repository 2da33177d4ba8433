"""Block masks (256 query rows x 64 keys) on the native gfx950 attention
kernels.

Reference for every numerics check: ops.reference.attention on fp32 copies
with the same masks, at the tolerance of the other attention tests
(rtol = atol = 2e-2).
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

BF16 = torch.bfloat16
F16 = torch.float16
RTOL = ATOL = 2e-2
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
DIMS = pytest.mark.parametrize("D", [64, 128])


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available("pack_block_lists"), (
        "native _pa_hip extension with the block-list kernels must be present"
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


def _ref(q, k, v, block, keys=None, scale=None):
    """fp32 reference on [B, H, S, D]."""
    return R.attention(q.float(), k.float(), v.float(), scale, key_mask=keys,
                       block_mask=block)


def _ref_bshd(q, k, v, block, keys=None, scale=None):
    return _ref(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                v.permute(0, 2, 1, 3), block, keys, scale).permute(0, 2, 1, 3)


def _from_lists(lists, nk):
    """Block mask with query block i attending the tiles lists[i]."""
    m = torch.zeros(len(lists), nk, dtype=torch.bool)
    for i, tiles in enumerate(lists):
        m[i, list(tiles)] = True
    return m.cuda()


def _nan_rows(t, rows):
    """t [B, H, Sk, D] with NaN at the key rows `rows` [B, Sk] marks."""
    return t.masked_fill(rows[:, None, :, None].expand_as(t), float("nan"))


def _unseen_keys(block, Sq, Sk, B, keys=None):
    """[B, Sk]: keys no query row of the batch element sees."""
    seen = block.any(dim=0).repeat_interleave(64)[:Sk][None].expand(B, Sk)
    if keys is not None:
        seen = seen & keys
    return ~seen


# ---------------- patterns ----------------

def _col_block(nq, nk):
    """The query block each tile falls into when both axes span the same
    sequence."""
    return (torch.arange(nk) * nq) // nk


def all_true(nq, nk):
    return torch.ones(nq, nk, dtype=torch.bool)


def band(nq, nk):
    return _col_block(nq, nk)[None, :] == torch.arange(nq)[:, None]


def lower_tri(nq, nk):
    return _col_block(nq, nk)[None, :] <= torch.arange(nq)[:, None]


def bernoulli(nq, nk):
    g = torch.Generator(device="cpu").manual_seed(100 * nq + nk)
    return torch.rand(nq, nk, generator=g) < 0.5


PATTERNS = (all_true, band, lower_tri, bernoulli)


# ---------------- shape and pattern sweep ----------------

@pytest.mark.parametrize("Sk", [64, 130, 321])
@pytest.mark.parametrize("Sq", [200, 257, 600])
@DTYPES
@DIMS
def test_block_mask_sweep(D, dtype, Sq, Sk, no_fallback):
    nq, nk = R.block_mask_shape(Sq, Sk)
    for H in (2, 4):  # B*H = 4: 2-D grid; 8: XCD-affine 1-D grid
        q = _randn(2, H, Sq, D, dtype=dtype, seed=1)
        k = _randn(2, H, Sk, D, dtype=dtype, seed=2)
        v = _randn(2, H, Sk, D, dtype=dtype, seed=3)
        for p in PATTERNS:
            block = p(nq, nk).cuda()
            out = ops.attention(q, k, v, block_mask=block)
            assert out.dtype == dtype and out.shape == q.shape
            _cmp(out, _ref(q, k, v, block),
                 f"{p.__name__} H={H} D={D} Sq={Sq} Sk={Sk}")


# ---------------- per-query-block trip counts ----------------

@pytest.mark.parametrize("lists", [
    ((), (6,)),                      # 0 tiles | the partial last tile alone
    ((0, 3), (1, 4, 6)),             # 2 and 3 tiles, none adjacent
    ((0, 2, 3, 5, 6), ()),           # 5 tiles | 0 tiles
], ids=["0|1", "2|3", "5|0"])
@DTYPES
@DIMS
def test_per_query_block_trip_counts(D, dtype, lists, no_fallback):
    """Sq=300 (two query blocks), Sk=401 (seven tiles, the last 17 keys):
    0, 1, 2, 3 and 5 live tiles — the prologue's nt > 1 guard and the D=128
    j+2 prefetch — with NaN in every tile a batch element never visits."""
    B, H, Sq, Sk = 2, 2, 300, 401
    block = _from_lists(lists, 7)
    q = _randn(B, H, Sq, D, dtype=dtype, seed=4)
    k = _randn(B, H, Sk, D, dtype=dtype, seed=5)
    v = _randn(B, H, Sk, D, dtype=dtype, seed=6)
    dead = _unseen_keys(block, Sq, Sk, B)
    out = ops.attention(q, _nan_rows(k, dead), _nan_rows(v, dead),
                        block_mask=block)
    bm = ops.pack_block_mask(block, B, Sq, Sk)
    assert bm.nlive.tolist() == [[len(t) for t in lists]] * B
    for i, tiles in enumerate(lists):
        assert bm.live[0, i, :len(tiles)].tolist() == list(tiles)
    _cmp(out, _ref(q, k, v, block), f"live tiles {lists}")
    for i, tiles in enumerate(lists):
        rows = out[:, :, 256 * i:256 * (i + 1)]
        if tiles:
            assert rows.float().abs().amax(-1).min() > 0, "live block is zero"
        else:
            assert torch.equal(rows, torch.zeros_like(rows))


# ---------------- all-true block mask ----------------

@pytest.mark.parametrize("H", [2, 4])
@DTYPES
@DIMS
def test_all_true_block_mask_equals_all_true_key_mask(D, dtype, H, no_fallback):
    """The tile sequence is the one the key-mask kernel walks: bitwise."""
    B, Sq, Sk = 2, 600, 321
    q = _randn(B, H, Sq, D, dtype=dtype, seed=7)
    k = _randn(B, H, Sk, D, dtype=dtype, seed=8)
    v = _randn(B, H, Sk, D, dtype=dtype, seed=9)
    keys = torch.ones(B, Sk, dtype=torch.bool, device="cuda")
    block = all_true(3, 6).cuda()
    assert torch.equal(ops.attention(q, k, v, block_mask=block),
                       ops.attention(q, k, v, key_mask=keys))


# ---------------- composition with a key mask ----------------

@DTYPES
@DIMS
def test_block_mask_composes_with_key_mask(D, dtype, no_fallback):
    """Tile 2 is block-live for query block 0, but element 1's key mask
    kills all of it: it must leave element 1's list, or its NaN K/V (for
    element 1 only) and the all-dead tile's sentinel arithmetic poison the
    row. Tile 4 is visited by nobody and NaN for everybody; dead keys of
    live tiles are NaN too."""
    B, H, Sq, Sk = 2, 2, 300, 401
    block = _from_lists(((0, 2, 5), (2, 3, 6)), 7)
    g = torch.Generator(device="cpu").manual_seed(10)
    keys = (torch.rand(B, Sk, generator=g) < 0.7).cuda()
    keys[1, 128:192] = False
    keys[0, 128:192] = True
    q = _randn(B, H, Sq, D, dtype=dtype, seed=11)
    k = _randn(B, H, Sk, D, dtype=dtype, seed=12)
    v = _randn(B, H, Sk, D, dtype=dtype, seed=13)
    dead = _unseen_keys(block, Sq, Sk, B, keys)
    assert dead[1, 128:192].all() and not dead[0, 128:192].any()
    assert dead[:, 256:320].all()
    kn, vn = _nan_rows(k, dead), _nan_rows(v, dead)
    bm = ops.pack_block_mask(block, B, Sq, Sk, key_mask=keys)
    assert bm.nlive.tolist() == [[3, 3], [2, 2]]
    assert bm.live[1, :, :2].tolist() == [[0, 5], [3, 6]]
    ref = _ref(q, k, v, block, keys)
    for what, out in (
            ("packed", ops.attention(q, kn, vn, block_mask=bm)),
            ("raw", ops.attention(q, kn, vn, key_mask=keys, block_mask=block)),
            ("raw + KeyMask", ops.attention(
                q, kn, vn, key_mask=ops.pack_key_mask(keys),
                block_mask=block.int()))):
        assert torch.isfinite(out.float()).all(), what
        _cmp(out, ref, what)
    with pytest.raises(ValueError, match="belongs in the pack"):
        ops.attention(q, k, v, key_mask=keys, block_mask=bm)


# ---------------- call routes ----------------

@DTYPES
def test_block_mask_bshd_strided_views(dtype, no_fallback):
    B, S, H, D = 2, 300, 4, 128
    qkv = _randn(B, S, 3, H, D, dtype=dtype, seed=14)
    q, k, v = qkv.unbind(2)  # strided views of a fused projection
    block = _from_lists(((0, 4), (1, 2, 3)), 5)
    out = ops.attention_bshd(q, k, v, block_mask=block)
    _cmp(out, _ref_bshd(q, k, v, block), "block mask, bshd strided")


@DIMS
def test_block_mask_cross_lengths(D, no_fallback):
    B, H = 2, 4
    q = _randn(B, 300, H, D, seed=15)
    k = _randn(B, 130, H, D, seed=16)
    v = _randn(B, 130, H, D, seed=17)
    block = _from_lists(((0, 2), (1,)), 3)
    bm = ops.pack_block_mask(block, B, 300, 130)
    ref = _ref_bshd(q, k, v, block)
    _cmp(ops.attention_bshd(q, k, v, block_mask=bm), ref, "cross, packed")
    _cmp(ops.attention_bshd(q, k, v, block_mask=block.long()), ref,
         "cross, raw int64 mask")


@DTYPES
def test_block_mask_split_outputs(dtype, no_fallback):
    B, S, H, D = 2, 320, 4, 128
    q = _randn(B, S, H, D, dtype=dtype, seed=18)
    k = _randn(B, S, H, D, dtype=dtype, seed=19)
    v = _randn(B, S, H, D, dtype=dtype, seed=20)
    block = _from_lists(((0, 1, 4), (2,)), 5)
    a, b = ops.attention_bshd_split(q, k, v, 100, block_mask=block)
    assert a.shape == (B, 100, H, D) and b.shape == (B, S - 100, H, D)
    assert a.is_contiguous() and b.is_contiguous()
    full = ops.attention_bshd(q, k, v, block_mask=block)
    assert torch.equal(a, full[:, :100])  # same kernel math: bitwise
    assert torch.equal(b, full[:, 100:])
    _cmp(torch.cat([a, b], 1), _ref_bshd(q, k, v, block), "block mask split")


def test_block_mask_pad_head_dim(no_fallback):
    B, S, H, D = 2, 300, 4, 40
    q = _randn(B, S, H, D, seed=21)
    k = _randn(B, 130, H, D, seed=22)
    v = _randn(B, 130, H, D, seed=23)
    block = _from_lists(((1,), (0, 2)), 3)
    out = ops.attention_bshd(q, k, v, block_mask=block)
    assert out.shape == q.shape
    _cmp(out, _ref_bshd(q, k, v, block), "block mask, pad route D=40")
    a, b = ops.attention_bshd_split(q, k, v, 50, block_mask=block)
    assert torch.equal(torch.cat([a, b], 1), out)


def test_fp32_gpu_block_mask_takes_reference_path(monkeypatch):
    """fp32 has no native instantiation: reference path, mask honoured, and
    the one-time note is given."""
    noted = []
    monkeypatch.setattr(ops, "_unsupported",
                        lambda op, why: noted.append((op, why)))
    q = _randn(2, 2, 300, 64, dtype=torch.float32, seed=24)
    k = _randn(2, 2, 130, 64, dtype=torch.float32, seed=25)
    v = _randn(2, 2, 130, 64, dtype=torch.float32, seed=26)
    block = _from_lists(((0,), ()), 3)
    out = ops.attention(q, k, v, block_mask=block)
    torch.testing.assert_close(out, _ref(q, k, v, block), rtol=0, atol=1e-5)
    assert torch.equal(out[:, :, 256:], torch.zeros_like(out[:, :, 256:]))
    assert noted and noted[0][0] == "attn_fwd"


# ---------------- pack_block_mask ----------------

def _expected_lists(block, words):
    """live / nlive from the definition, on the CPU."""
    block, words = block.cpu(), words.cpu()
    alive = block[None] & (words != 0)[:, None]          # [B, nq, nk]
    live = torch.zeros(alive.shape, dtype=torch.int32)
    for b in range(alive.shape[0]):
        for i in range(alive.shape[1]):
            idx = alive[b, i].nonzero().flatten().int()
            live[b, i, :len(idx)] = idx
    return live, alive.sum(-1).int()


@pytest.mark.parametrize("Sq,Sk", [(200, 64), (600, 321), (256, 4480),
                                   (700, 4480 + 9)])
@pytest.mark.parametrize("with_keys", [False, True], ids=["block", "block+keys"])
def test_pack_block_mask_outputs(Sq, Sk, with_keys):
    """live, nlive and the zero-filled tails equal a torch computation;
    Sk = 4480 is 70 tiles, a second 64-tile compaction step. The key mask
    empties whole tiles for one element or the other."""
    B = 3
    nq, nk = R.block_mask_shape(Sq, Sk)
    g = torch.Generator(device="cpu").manual_seed(Sq + Sk)
    block = torch.rand(nq, nk, generator=g) < 0.6
    if nq > 1:
        block[-1] = False
    keys = None
    if with_keys:
        keys = torch.rand(B, Sk, generator=g) < 0.5
        tiles_off = torch.rand(B, nk, generator=g) < 0.4
        keys &= ~tiles_off.repeat_interleave(64, dim=1)[:, :Sk]
        keys[2] = False                                   # an empty element
        keys = keys.cuda()
    bm = ops.pack_block_mask(block.cuda().to(torch.uint8) * 3, B, Sq, Sk,
                             key_mask=keys)
    want_words = ops.pack_key_mask(
        keys if with_keys else torch.ones(B, Sk, dtype=torch.bool,
                                          device="cuda")).words
    assert bm.block.dtype == torch.bool and torch.equal(bm.block.cpu(), block)
    assert (bm.keys is None) == (not with_keys)
    assert bm.words.dtype == torch.int64 and bm.live.dtype == torch.int32
    assert bm.nlive.dtype == torch.int32
    assert bm.live.shape == (B, nq, nk) and bm.nlive.shape == (B, nq)
    assert torch.equal(bm.words, want_words)
    if not with_keys and Sk % 64:
        # bits at or beyond Sk are 0
        assert bm.words[:, -1].tolist() == [(1 << (Sk % 64)) - 1] * B
    live, nlive = _expected_lists(block, bm.words)
    assert torch.equal(bm.nlive.cpu(), nlive)
    assert torch.equal(bm.live.cpu(), live)
    assert (bm.batch, bm.Sq, bm.Sk) == (B, Sq, Sk)


def test_float_block_mask_raises_on_gpu():
    m = all_true(1, 1).cuda()
    with pytest.raises(ValueError, match="additive"):
        ops.pack_block_mask(m.float(), 1, 64, 64)
    words = ops.pack_key_mask(torch.ones(1, 64, dtype=torch.bool,
                                         device="cuda")).words
    with pytest.raises(RuntimeError, match="additive"):
        ops.hip_ext().pack_block_lists(m.float(), words)
    with pytest.raises(RuntimeError, match="key tiles"):
        ops.hip_ext().pack_block_lists(all_true(1, 2).cuda(), words)


def test_launcher_rejects_lists_packed_for_another_problem():
    ext = ops.hip_ext()
    B, Sq, Sk = 2, 300, 130
    q = _randn(B, Sq, 2, 64, seed=27)
    k = _randn(B, Sk, 2, 64, seed=28)

    def packed(b, sq, sk):
        return ops.pack_block_mask(all_true(*R.block_mask_shape(sq, sk)).cuda(),
                                   b, sq, sk)

    args = (q, k, k, 0.125)
    bm = packed(B, Sq, Sk)
    ext.attn_fwd_bshd_masked(*args, bm.words, bm.live, bm.nlive)
    for other, msg in (((3, Sq, Sk), "batch"), ((B, 600, Sk), "another Sq"),
                       ((B, 200, Sk), "another Sq"),
                       ((B, Sq, 321), "another Sk")):
        o = packed(*other)
        with pytest.raises(RuntimeError, match=msg):
            ext.attn_fwd_bshd_masked(*args, o.words, o.live, o.nlive)
        with pytest.raises(ValueError, match="packed for"):
            ops.attention_bshd(q, k, k, block_mask=o)
    with pytest.raises(RuntimeError, match="int32 live"):
        ext.attn_fwd_bshd_masked(*args, bm.words, bm.live.long(), bm.nlive)
    with pytest.raises(RuntimeError, match="batch"):
        ext.attn_fwd_bshd_masked(*args, bm.words, bm.live, bm.nlive[:, 0])
    with pytest.raises(RuntimeError, match="device"):
        ext.attn_fwd_bshd_masked(*args, bm.words, bm.live.cpu(), bm.nlive)
    # same tile counts, other lengths: caught before launch by the op
    with pytest.raises(ValueError, match="packed for"):
        ops.attention_bshd(q, k, k, block_mask=packed(B, Sq, Sk - 1))


# ---------------- graph replay ----------------

def test_block_mask_graph_replay(no_fallback):
    """Capture both packs + attention; replay after copying another block
    mask into the static buffer: the result follows it (no host read)."""
    B, S, H, D = 2, 300, 4, 128
    q = _randn(B, S, H, D, seed=29)
    k = _randn(B, S, H, D, seed=30)
    v = _randn(B, S, H, D, seed=31)
    mask_a = _from_lists(((0, 4), (1, 2, 3)), 5)
    mask_b = _from_lists(((2,), (0, 1, 3, 4)), 5)
    static_mask = mask_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention_bshd(q, k, v, block_mask=static_mask)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = ops.attention_bshd(q, k, v, block_mask=static_mask)
    graph.replay()
    _cmp(static_out, _ref_bshd(q, k, v, mask_a), "replay, captured mask")
    static_mask.copy_(mask_b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out,
                       ops.attention_bshd(q, k, v, block_mask=mask_b))
    _cmp(static_out, _ref_bshd(q, k, v, mask_b), "replay, new mask")


# ---------------- whole model ----------------

def test_wan_frame_window_gpu_vs_cpu_reference(no_fallback):
    """WanDiT.tiny() with self_attn_frame_window=0 on [2, 4, 6, 16, 16]
    (f=6, 64 tokens a frame: block 0 sees frames 0-3, block 1 frames 4-5):
    bf16 native kernels on GPU against the same weights in fp32 on the CPU
    reference path, at test_whole_model_masked_gpu_vs_cpu_reference's
    bound."""
    from comfyui_parallelanything_amd.models.wan import WanConfig, WanDiT

    cfg = WanConfig.tiny()
    cfg.self_attn_frame_window = 0
    torch.manual_seed(0)
    m_ref = WanDiT(cfg).float().eval()
    m_gpu = copy.deepcopy(m_ref).to("cuda", BF16)
    dense_cfg = copy.copy(cfg)
    dense_cfg.self_attn_frame_window = None
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(2, 4, 6, 16, 16, generator=g)
    t = torch.rand(2, generator=g)
    c = torch.randn(2, 8, 32, generator=g)
    with torch.no_grad():
        ref = m_ref(x, t, context=c).float()
        m_ref.cfg = dense_cfg
        dense = m_ref(x, t, context=c).float()
        out = m_gpu(x.cuda().bfloat16(), t.cuda(),
                    context=c.cuda().bfloat16()).float().cpu()
    assert len(m_gpu._mask_cache) == 1
    bm = next(iter(m_gpu._mask_cache.values()))
    assert bm.nlive.tolist() == [[4, 2]] * 2
    assert (dense - ref).abs().max() > 1e-3, "mask had no effect"
    rel = (out - ref).norm() / ref.norm()
    assert rel < 0.15, f"whole-model rel-l2 {rel:.4f}"
    corr = torch.corrcoef(torch.stack([out.flatten(), ref.flatten()]))[0, 1]
    assert corr > 0.99, f"correlation {corr:.4f}"
