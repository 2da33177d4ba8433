"""Native gfx950 attention on inputs where a phantom key shows.

The other attention files feed randn, where a dead key that wrongly enters
the softmax (score 0, V = 0) weighs about 1/Sk and hides under rtol = atol =
2e-2. Here every real score is about -6 (negative_scores: the phantom takes a
quarter of the softmax or more) or the correct output is exactly 1.0 or 0.0
(uniform_ones). Inputs, masks and shapes come from kernel_cases.py;
test_kernel_cases_reference.py proves on the CPU that they reject a skipped
sentinel at each of the 64 bit positions, a tail bound off by one, `full`
taken on a partial tile and a skipped alpha rescale.

Reference for every numerics check: ops.reference.attention on fp32 copies,
at the tolerance of the other attention tests.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_cases as C
from comfyui_parallelanything_amd import ops

DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DIMS = pytest.mark.parametrize("D", C.DIMS)
REGIMES = pytest.mark.parametrize("regime", list(C.ATTN_BUILDERS))


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


# each case and its fp32 reference are built once and never modified
@functools.lru_cache(maxsize=None)
def _case(kind, *args):
    case = getattr(C, kind + "_case")(*args)
    return case, C.attn_ref(case)


def _cuda(t):
    return None if t is None else t.cuda()


def _run(case, layout="bhsd", split=None, scale=None):
    """The case through ops.attention ([B, H, S, D] out), or through
    attention_bshd / attention_bshd_split on permuted views."""
    q, k, v = (_cuda(case[n]) for n in "qkv")
    kw = dict(key_mask=_cuda(case["keys"]), block_mask=_cuda(case["block"]))
    if layout == "bhsd":
        return ops.attention(q, k, v, scale, **kw)
    q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    if split is None:
        out = ops.attention_bshd(q, k, v, scale, **kw)
    else:
        a, b = ops.attention_bshd_split(q, k, v, split, scale, **kw)
        assert a.shape[1] == split and a.is_contiguous() and b.is_contiguous()
        out = torch.cat([a, b], dim=1)
    return out.permute(0, 2, 1, 3)


def _exact_ones(out, case, what):
    """uniform_ones: exactly 1.0 where the row sees a key, exactly 0.0
    where it sees none."""
    seen = C.visibility(case).any(-1)[:, None, :, None].expand(out.shape)
    want = seen.to(out.dtype)
    got = out.cpu()
    assert torch.equal(got, want), (
        f"{what}: {(got != want).sum().item()} of {got.numel()} values are "
        f"not exactly 1/0; range of the wrong ones "
        f"{got[got != want].float().min().item()} .. "
        f"{got[got != want].float().max().item()}")


# ---------------- unmasked tail ----------------

@pytest.mark.parametrize("Sk", C.TAIL_SK + (C.CONTROL_SK,))
@DT
@DIMS
def test_unmasked_tail(D, dtype, Sk, no_fallback):
    """`key < Sk` against `kv0 + 64 <= Sk`: one key, one short of a tile,
    one over, three tiles and one key; Sk=128 is the all-full control. One
    and two query blocks."""
    for Sq in C.TAIL_SQ:
        case, ref = _case("tail", "negative_scores", D, dtype, Sq, Sk)
        out = _run(case)
        assert out.dtype == dtype
        C.check(out, ref, what=f"negative_scores Sq={Sq} Sk={Sk}")
        case, _ = _case("tail", "uniform_ones", D, dtype, Sq, Sk)
        out = _run(case)
        assert torch.equal(out.cpu(), torch.ones_like(case["q"])), \
            f"uniform_ones Sq={Sq} Sk={Sk}: min {out.float().min().item()}"


@pytest.mark.parametrize("poison", [float("nan"), 3e4], ids=["nan", "3e4"])
@pytest.mark.parametrize("Sk", C.OVERREAD_SK)
@DT
@DIMS
def test_tail_does_not_read_past_sk(D, dtype, Sk, poison, no_fallback):
    """K and V are the first Sk rows of buffers 64 rows longer, and the rest
    is poison: the last tile is staged and scored from rows below Sk only.
    Bit-equal to the same call on exact-size tensors."""
    case, ref = _case("tail", "negative_scores", D, dtype, 40, Sk)
    q, k, v = (case[n].cuda().permute(0, 2, 1, 3).contiguous() for n in "qkv")
    B, _, H, _ = k.shape
    kbuf = torch.full((B, Sk + 64, H, D), poison, dtype=dtype, device="cuda")
    vbuf = torch.full((B, Sk + 64, H, D), poison, dtype=dtype, device="cuda")
    kbuf[:, :Sk] = k
    vbuf[:, :Sk] = v
    exact = ops.attention_bshd(q, k, v)
    out = ops.attention_bshd(q, kbuf[:, :Sk], vbuf[:, :Sk])
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, exact)
    C.check(out.permute(0, 2, 1, 3), ref, what=f"over-read Sk={Sk}")


# ---------------- key masks ----------------

@pytest.mark.parametrize("Sk", C.MASK_SK)
@REGIMES
@DT
@DIMS
def test_key_masks(D, dtype, regime, Sk, no_fallback):
    """Bernoulli, hole, one-in-last-tile, a single dead key per tile at a
    walking bit position, and an empty batch element, in one call."""
    case, ref = _case("mask", regime, D, dtype, Sk)
    out = _run(case)
    empty = C.key_mask_stack(Sk).any(-1).logical_not().nonzero().flatten()
    assert empty.tolist() == [4]
    assert torch.equal(out[4], torch.zeros_like(out[4])), "empty element"
    if regime == "uniform_ones":
        _exact_ones(out, case, f"Sk={Sk}")
    else:
        names = ("bernoulli", "hole", "one_in_last_tile", "walking_dead")
        for b, name in enumerate(names):
            C.check(out[b], ref[b], what=f"{name} Sk={Sk}")


# ---------------- block masks composed with a key mask ----------------

@REGIMES
@DT
@DIMS
def test_block_mask_with_key_mask(D, dtype, regime, no_fallback):
    """Sq=600, Sk=321: per-query-block live lists of different lengths over
    Bernoulli key words; query block 2 and the rows a key mask blinds see
    nothing and give exact zeros."""
    case, ref = _case("block", regime, D, dtype)
    out = _run(case)
    blind = ~C.visibility(case).any(-1)                    # [B, Sq]
    assert blind.any()
    got = out.cpu()
    rows = blind[:, None, :, None].expand(got.shape)
    assert torch.equal(got[rows], torch.zeros_like(got[rows])), "blind rows"
    if regime == "uniform_ones":
        _exact_ones(out, case, "block x keys")
    else:
        C.check(out, ref, what="block x keys")


# ---------------- other routes and regimes ----------------

@DT
@DIMS
def test_split_route_masked(D, dtype, no_fallback):
    case, ref = _case("mask", "negative_scores", D, dtype, 193)
    out = _run(case, layout="bshd", split=100)
    C.check(out, ref, what="attention_bshd_split")
    assert torch.equal(out[4], torch.zeros_like(out[4]))


@DT
@pytest.mark.parametrize("D", C.PAD_DIMS)
def test_pad_route_masked(D, dtype, no_fallback):
    """D=40/80 zero-padded to 64/128; the scale is that of the unpadded D."""
    case, ref = _case("mask", "negative_scores", D, dtype, C.PAD_SK)
    out = _run(case, layout="bshd")
    assert out.shape[-1] == D
    C.check(out, ref, what=f"pad route D={D}")
    assert torch.equal(out[4], torch.zeros_like(out[4]))


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "alltrue"])
@pytest.mark.parametrize("reverse", [False, True], ids=["rising", "falling"])
@DT
@DIMS
def test_staircase(D, dtype, reverse, masked, no_fallback):
    """Rising: the running maximum grows on every tile, the accumulators are
    rescaled each time. Falling: it never grows after tile 0, alpha == 1 and
    the rescale is skipped each time."""
    case, ref = _case("staircase", D, dtype, reverse, masked)
    C.check(_run(case), ref, what="staircase")


@pytest.mark.parametrize("scale", [-0.125, 0.0])
@pytest.mark.parametrize("layout", ["bhsd", "bshd", "split"])
def test_nonpositive_scale_matches_or_raises(layout, scale):
    """The kernels take the maximum of the raw scores and scale it
    afterwards, and their dead-key sentinel is a large negative raw score:
    both need scale > 0. ops refuses anything else; were it ever let
    through, it would have to match the reference."""
    case, _ = _case("tail", "negative_scores", 64, C.BF16, 40, 65)
    try:
        out = _run(case, layout="bshd" if layout == "split" else layout,
                   split=20 if layout == "split" else None, scale=scale)
    except ValueError as err:
        assert "scale" in str(err)
        return
    C.check(out, C.attn_ref(case, scale), what=f"scale={scale}")
