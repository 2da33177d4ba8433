"""Native gfx950 attention held to its rounding model.

The other attention files accept rtol = atol = 2e-2, which passes a kernel
that truncates P, rounds its accumulators or its scores to 16 bit, or folds a
rounded scale. Here the kernels run through the three kinds of case of
attention_cases.py (docs/KERNELS.md, "Attention accuracy contract"):
constant V columns and one-hot gathers, whose outputs are known bit for bit,
and random data against fp64 by rho = rms(err / sigma) and a rigorous
per-element bound. test_attention_cases_reference.py proves on the CPU that
these checks reject each arithmetic fault and accept the emulation.

Also here: the launcher's refusals (k or v of another batch, head count or
head dim than q, a split outside the rows), the alignment copies and the
empty shapes.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A
import kernel_cases as C
from comfyui_parallelanything_amd import ops
from test_gpu_attn_regimes import no_fallback, require_ext  # noqa: F401

DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DIMS = pytest.mark.parametrize("D", C.DIMS)
PADS = pytest.mark.parametrize("D", C.PAD_DIMS)
GRID = pytest.mark.parametrize("grid", A.GRIDS, ids=A.GRID_IDS)
QMUL = pytest.mark.parametrize("qmul", A.Q_SCALES, ids=["q1", "q3"])
MASK = pytest.mark.parametrize("mask", [None, "keys"],
                               ids=["unmasked", "bernoulli"])
XCD = A.GRIDS[0]


# every case is built once and never modified
@functools.lru_cache(maxsize=None)
def _constant(*args, **kw):
    return A.constant_columns(*args, **dict(kw))


@functools.lru_cache(maxsize=None)
def _gather(*args):
    return A.one_hot_gather(*args)


def _run(case, route="bhsd", scale=None):
    return A.run_ops(case, route, "cuda", scale)


# ------------------------------------------------------ a. constant_columns

@MASK
@QMUL
@GRID
@DT
@DIMS
def test_constant_columns(D, dtype, grid, qmul, mask, no_fallback):
    """Through ops.attention, on both grids."""
    case = _constant(*grid, D, dtype, qmul, mask=mask)
    out = _run(case)
    assert out.dtype == dtype
    A.check_constant(out, case, f"{grid} q*{qmul} {mask}")


@QMUL
@DT
@DIMS
def test_constant_columns_block_mask(D, dtype, qmul, no_fallback):
    """kernel_cases.block_case's masks: per-query-block live lists over
    Bernoulli key words, and rows that see nothing, exactly +0."""
    case = _constant(0, 0, D, dtype, qmul, mask="block")
    A.check_constant(_run(case), case, "block x keys")


@MASK
@DT
@DIMS
def test_constant_columns_bshd_routes(D, dtype, mask, no_fallback):
    """attention_bshd on the three strided views of one [B, S, 3, H, D]
    buffer (S = 321), and attention_bshd_split at 7 (inside the first wave)
    and 256 (the query-block boundary) on permuted tensors."""
    case = _constant(*XCD, D, dtype, 3.0, Sq=A.FUSED_S, mask=mask)
    A.check_constant(_run(case, "fused"), case, "fused views")
    case = _constant(*XCD, D, dtype, 3.0, mask=mask)
    for route in ("bshd", "split7", "split256"):
        A.check_constant(_run(case, route), case, route)


@MASK
@DT
@PADS
def test_constant_columns_pad_route(D, dtype, mask, no_fallback):
    """D = 40 / 80, zero-padded to 64 / 128 by attention_bshd."""
    for grid in A.GRIDS:
        case = _constant(*grid, D, dtype, 3.0, mask=mask)
        out = _run(case, "bshd")
        assert out.shape[-1] == D
        A.check_constant(out, case, f"pad D={D} {grid}")


@pytest.mark.parametrize("layout", ["dim_offset", "batch_stride"])
@DT
@DIMS
def test_constant_columns_on_unaligned_views(D, dtype, layout, no_fallback):
    """[..., 4:4+D] views (an 8-byte aligned base) and a batch stride of
    D*H*S + 4: the launcher copies both, so the kernel's 16-byte loads see
    aligned tensors whatever the hardware would accept."""
    case = _constant(*XCD, D, dtype, 3.0, mask="keys")
    B, H = XCD

    def view(t):
        t = t.permute(0, 2, 1, 3).cuda()                   # [B, S, H, D]
        S = t.shape[1]
        if layout == "dim_offset":
            buf = torch.full((B, S, H, D + 8), float("nan"), dtype=dtype,
                             device="cuda")
            out = buf[..., 4:4 + D]
            assert out.data_ptr() % 16 == 8
        else:
            n = S * H * D
            buf = torch.full((B * (n + 4),), float("nan"), dtype=dtype,
                             device="cuda")
            out = buf.as_strided((B, S, H, D), (n + 4, H * D, D, 1))
            assert out.stride(0) % 8 == 4
        out.copy_(t)
        return out

    q, k, v = (view(case[n]) for n in "qkv")
    out = ops.attention_bshd(q, k, v, key_mask=case["keys"].cuda())
    A.check_constant(out.permute(0, 2, 1, 3), case, layout)


# -------------------------------------------------------- b. one_hot_gather

@pytest.mark.parametrize("variant", A.GATHER_VARIANTS)
@GRID
@DT
@DIMS
def test_one_hot_gather(D, dtype, grid, variant, no_fallback, record_property):
    """Key j, dim d of V arrives unaltered at row i, dim d of O: every
    normal pattern bit for bit, a subnormal as itself or zero."""
    case = _gather(variant, *grid, D, dtype)
    seen = A.check_gather(_run(case), case, f"{variant} {grid}")
    print(f"one_hot_gather {variant} D={D} {dtype} {grid}: {seen}")
    record_property("subnormals_and_zeros", str(seen))


@pytest.mark.parametrize("variant", ["rising", "dead_twin"])
@DT
@PADS
def test_one_hot_gather_pad_route(D, dtype, variant, no_fallback):
    case = _gather(variant, *XCD, D, dtype)
    A.check_gather(_run(case, "bshd"), case, f"{variant} pad D={D}")


# -------------------------------------------------------- c. rounding_model

@pytest.mark.parametrize("scale", A.MODEL_SCALES, ids=["default", "s0.3"])
@pytest.mark.parametrize("regime", A.MODEL_REGIMES)
@GRID
@DT
@DIMS
def test_rounding_model(D, dtype, grid, regime, scale, no_fallback):
    """rho within RHO_MARGIN of the emulation's own rho for the case, and
    no element beyond the rigorous bound."""
    case, r, rho = A.model_case(regime, grid, D, dtype, scale)
    A.check_model(_run(case, scale=scale), r, dtype, A.RHO_MARGIN * rho,
                  f"{regime} D={D} {dtype} {grid} scale={scale} "
                  f"(emulation {rho:.4f})")


# ----------------------------------------------------- refusals and empties

@pytest.fixture()
def no_launch(monkeypatch):
    """Fails the test if a refused call reaches the extension."""
    calls = []
    orig = ops._attn_native

    def spy(*a, **kw):
        calls.append(a[0].shape)
        return orig(*a, **kw)

    monkeypatch.setattr(ops, "_attn_native", spy)
    yield calls


def _bshd(B=2, S=40, H=4, D=64, dtype=C.BF16):
    g = torch.Generator(device="cpu").manual_seed(3)
    return [torch.randn(B, S, H, D, generator=g).to(dtype).cuda()
            for _ in range(3)]


# too-small k / v as views into full-size buffers: a build that did not
# refuse would index past the view, inside the buffer
SMALL = {
    "batch": (lambda t: t[:1], "batch"),
    "heads": (lambda t: t[:, :, :3], "heads"),
    "head dim": (lambda t: t[..., :64], "head dim"),
}


@pytest.mark.parametrize("which", ["k", "v", "kv"])
@pytest.mark.parametrize("name", list(SMALL))
def test_mismatched_kv_is_refused(name, which, no_launch):
    cut, word = SMALL[name]
    D = 128 if name == "head dim" else 64
    q, k, v = _bshd(D=D)
    ks = cut(k) if "k" in which else k
    vs = cut(v) if "v" in which else v
    mask = torch.ones(2, 40, dtype=torch.bool, device="cuda")
    for kw in (dict(), dict(key_mask=mask)):
        with pytest.raises(ValueError, match=word):
            ops.attention_bshd(q, ks, vs, **kw)
        with pytest.raises(ValueError, match=word):
            ops.attention_bshd_split(q, ks, vs, 7, **kw)
        with pytest.raises(ValueError, match=word):
            ops.attention(*(t.permute(0, 2, 1, 3) for t in (q, ks, vs)), **kw)
    assert not no_launch, "a refused call reached the extension"
    # the launcher's own check, for callers of the extension
    ext = ops.hip_ext()
    with pytest.raises(RuntimeError, match=word):
        ext.attn_fwd_bshd(q, ks, vs, 0.125)
    with pytest.raises(RuntimeError, match=word):
        ext.attn_fwd(*(t.permute(0, 2, 1, 3) for t in (q, ks, vs)), 0.125)
    # no launch error is pending: a valid call next, and it is right
    out = ops.attention_bshd(q, k, v)
    C.check(out, ops.reference.attention(
        *(t.permute(0, 2, 1, 3).float().cpu() for t in (q, k, v))
    ).permute(0, 2, 1, 3), what="after the refusal")


@pytest.mark.parametrize("split", [0, 40, 45, -1])
def test_split_outside_the_rows_is_refused(split, no_launch):
    q, k, v = _bshd()
    with pytest.raises(ValueError, match="split"):
        ops.attention_bshd_split(q, k, v, split)
    assert not no_launch
    with pytest.raises(RuntimeError, match="split"):
        ops.hip_ext().attn_fwd_bshd_split(q, k, v, 0.125, split)
    a, b = ops.attention_bshd_split(q, k, v, 39)
    assert a.shape[1] == 39 and b.shape[1] == 1
    assert torch.equal(torch.cat([a, b], 1), ops.attention_bshd(q, k, v))


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("empty", ["B", "H", "Sq", "Sk"])
def test_empties(empty, masked, no_fallback):
    """B, H or Sq of zero: the empty result without a launch (a grid of
    zero blocks is a launch error). Sk = 0: zeros. A valid call follows."""
    dims = dict(B=2, H=4, Sq=40, Sk=70)
    dims[empty] = 0
    g = torch.Generator(device="cpu").manual_seed(4)
    q = torch.randn(dims["B"], dims["Sq"], dims["H"], 64, generator=g)
    k = torch.randn(dims["B"], dims["Sk"], dims["H"], 64, generator=g)
    q, k = q.to(C.F16).cuda(), k.to(C.F16).cuda()
    kw = {}
    if masked:
        kw["key_mask"] = torch.ones(dims["B"], dims["Sk"], dtype=torch.bool,
                                    device="cuda")
    want = torch.zeros_like(q)
    assert torch.equal(ops.attention_bshd(q, k, k, **kw), want)
    out = ops.attention(*(t.permute(0, 2, 1, 3) for t in (q, k, k)), **kw)
    assert torch.equal(out, want.permute(0, 2, 1, 3))
    if empty == "Sq":
        with pytest.raises(ValueError, match="split"):
            ops.attention_bshd_split(q, k, k, 7, **kw)
    else:
        a, b = ops.attention_bshd_split(q, k, k, 7, **kw)
        assert torch.equal(torch.cat([a, b], 1), want)
    torch.cuda.synchronize()
    q, k, v = _bshd()
    assert torch.isfinite(ops.attention_bshd(q, k, v).float()).all()
