"""Full-tile fast path of the native gfx950 attention kernels.

The KV loop skips the per-key validity work (key index, compare, select) on
a tile whose 64 keys are all live — every tile but a last partial one when
unmasked, every all-ones mask word when masked — and does it only on a tile
that can hold a dead key. These are the smallest shapes at which that choice
can go wrong: only full tiles, only a partial tile, tails of 1 and 63 keys,
partial tiles between full ones, and the D=128 pipeline's j+2 prefetch with
and without a tail.

Reference for every numerics check: ops.reference.attention on fp32 copies,
at the tolerances the other attention tests use (test_gpu_kernels.py for
bf16, test_gpu_fp16.py for fp16: rtol = atol = 2e-2).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

BF16 = torch.bfloat16
F16 = torch.float16
RTOL = ATOL = 2e-2
B, H = 2, 2
FULL_SK = [64, 128, 192, 256]
TAIL_SK = [1, 63, 65, 127, 129, 193]
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
DIMS = pytest.mark.parametrize("D", [64, 128])


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available("attn_fwd_bshd_masked"), (
        "native _pa_hip extension with the attention kernels must be present"
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


def _ref(q, k, v, mask=None):
    """fp32 reference on [B, H, S, D]."""
    return R.attention(q.float(), k.float(), v.float(), None, key_mask=mask)


def _ref_bshd(q, k, v, mask=None):
    return _ref(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                v.permute(0, 2, 1, 3), mask).permute(0, 2, 1, 3)


def _qkv(Sq, Sk, D, dtype, seed):
    return (_randn(B, H, Sq, D, dtype=dtype, seed=seed),
            _randn(B, H, Sk, D, dtype=dtype, seed=seed + 1),
            _randn(B, H, Sk, D, dtype=dtype, seed=seed + 2))


def _ones(Sk):
    return torch.ones(B, Sk, dtype=torch.bool, device="cuda")


# ---------------- unmasked: which tiles are full ----------------

@pytest.mark.parametrize("Sk", FULL_SK + TAIL_SK)
@DTYPES
@DIMS
def test_full_and_tail_tiles(D, dtype, Sk, no_fallback):
    """Sk % 64 == 0: every tile takes the fast path (192 and 256 run the
    D=128 j+2 prefetch on fast tiles only). Otherwise the last tile is
    partial: alone (1, 63), with a one-key tail (65, 129, 193) or a 63-key
    tail (127)."""
    q, k, v = _qkv(Sk, Sk, D, dtype, seed=100)
    out = ops.attention(q, k, v)
    assert out.dtype == dtype and out.shape == q.shape
    _cmp(out, _ref(q, k, v), f"D={D} Sk={Sk}")


@pytest.mark.parametrize("Sk", [128, 193])
@pytest.mark.parametrize("Sq", [40, 300])
@DTYPES
@DIMS
def test_cross_lengths_and_partial_q_blocks(D, dtype, Sq, Sk, no_fallback):
    """Sq != Sk; Sq = 40 is one partial q-block, 300 a full and a partial."""
    q, k, v = _qkv(Sq, Sk, D, dtype, seed=110)
    _cmp(ops.attention(q, k, v), _ref(q, k, v), f"D={D} Sq={Sq} Sk={Sk}")


@pytest.mark.parametrize("row", [180, 192], ids=["last_full_tile", "tail"])
@DTYPES
@DIMS
def test_forced_rescale_in_both_flavours(D, dtype, row, no_fallback):
    """Sk = 193: tiles 0-2 full, a one-key tail. One K row scaled x8 in the
    last full tile (key 180) or in the tail (key 192) makes the running max
    jump there for about half the query rows, so alpha != 1 rescales the
    accumulators in the full-tile flavour and in the partial one."""
    q, k, v = _qkv(300, 193, D, dtype, seed=120)
    k[:, :, row] *= 8
    _cmp(ops.attention(q, k, v), _ref(q, k, v), f"D={D} spike at {row}")


# ---------------- masked: which words are full ----------------

@pytest.mark.parametrize("Sk", [128, 130])
@DTYPES
@DIMS
def test_all_true_mask(D, dtype, Sk, no_fallback):
    """Sk = 128: both words are all ones, every tile is fast. Sk = 130: the
    last word has two bits and takes the per-key path."""
    q, k, v = _qkv(300, Sk, D, dtype, seed=130)
    out = ops.attention(q, k, v, key_mask=_ones(Sk))
    _cmp(out, _ref(q, k, v, _ones(Sk)), f"all-true D={D} Sk={Sk}")
    _cmp(out, _ref(q, k, v), "all-true vs unmasked reference")


@pytest.mark.parametrize("Sk", FULL_SK)
@DTYPES
@DIMS
def test_unmasked_equals_all_true_masked_bitwise(D, dtype, Sk, no_fallback):
    """With Sk % 64 == 0 the unmasked and the all-true-masked kernels run
    the same arithmetic on every tile (bitwise equal before the fast path
    existed too), so any difference is a wrong tile flavour."""
    q, k, v = _qkv(300, Sk, D, dtype, seed=140)
    assert torch.equal(ops.attention(q, k, v),
                       ops.attention(q, k, v, key_mask=_ones(Sk)))


@DTYPES
@DIMS
def test_partial_words_between_full_ones(D, dtype, no_fallback):
    """Sk = 192, three tiles. Element 0: a single live key in tile 1 between
    two full tiles (fast, per-key, fast). Element 1: tile 1 dead between two
    full tiles (never visited). A x8 K row at the single live key forces the
    rescale in the per-key flavour mid-sequence."""
    Sk = 192
    mask = _ones(Sk)
    mask[0, 64:128] = False
    mask[0, 100] = True
    mask[1, 64:128] = False
    q, k, v = _qkv(300, Sk, D, dtype, seed=150)
    k[0, :, 100] *= 8
    km = ops.pack_key_mask(mask)
    assert km.nlive.tolist() == [3, 2]
    assert km.live[1, :2].tolist() == [0, 2]
    _cmp(ops.attention(q, k, v, key_mask=km), _ref(q, k, v, mask),
         f"partial words D={D}")


@DIMS
def test_empty_element_next_to_full_tiles(D, no_fallback):
    """One batch element without a live key gives zeros; the other, all
    full words, is unaffected."""
    Sk = 128
    mask = _ones(Sk)
    mask[1] = False
    q, k, v = _qkv(300, Sk, D, BF16, seed=160)
    out = ops.attention(q, k, v, key_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(out[1], torch.zeros_like(out[1]))
    _cmp(out[0], _ref(q, k, v, mask)[0], "element beside the empty one")


# ---------------- split outputs ----------------

@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@DTYPES
def test_split_outputs_at_full_tile_sk(dtype, masked, no_fallback):
    """attention_bshd_split at Sk = 192 (full tiles only, BH = 16: XCD
    grid): out2 rows follow the same path as the joint output."""
    Bs, S, Hs, D = 2, 192, 8, 128
    q = _randn(Bs, S, Hs, D, dtype=dtype, seed=170)
    k = _randn(Bs, S, Hs, D, dtype=dtype, seed=171)
    v = _randn(Bs, S, Hs, D, dtype=dtype, seed=172)
    mask = torch.ones(Bs, S, dtype=torch.bool, device="cuda") if masked \
        else None
    a, b = ops.attention_bshd_split(q, k, v, 64, key_mask=mask)
    assert a.shape == (Bs, 64, Hs, D) and b.shape == (Bs, S - 64, Hs, D)
    full = ops.attention_bshd(q, k, v, key_mask=mask)
    assert torch.equal(a, full[:, :64])  # same kernel math: bitwise
    assert torch.equal(b, full[:, 64:])
    _cmp(torch.cat([a, b], 1), _ref_bshd(q, k, v, mask), "split, full tiles")
