"""Native gfx950 attention with a log-sum-exp output, the merge kernel and
the ring on top of them.

The LSE instantiations of attn_fwd_v4_kernel differ from the plain ones by
one store, so their out is the plain op's bit for bit and their lse is held
to the fp64 logsumexp by attn_lse_cases.py's bound. attn_merge_kernel goes
through the exact cases (constant columns, one-hot gathers, degenerate
partials) and the rounding model with one more rounding per partial.
test_attn_lse_reference.py proves on the CPU that these checks reject each
injected fault and accept the emulation.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A
import attn_lse_cases as L
import kernel_cases as C
from comfyui_parallelanything_amd import ops
from test_gpu_attn_regimes import no_fallback  # noqa: F401

DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DIMS = pytest.mark.parametrize("D", C.DIMS)
GRID = pytest.mark.parametrize("grid", A.GRIDS, ids=A.GRID_IDS)
CUTS = pytest.mark.parametrize("cuts", ["3", "8"])
BSHD = pytest.mark.parametrize("bshd", [False, True], ids=["bhsd", "bshd"])
XCD = A.GRIDS[0]


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for name in ("attn_fwd_lse", "attn_fwd_bshd_lse", "attn_fwd_lse_masked",
                 "attn_fwd_bshd_lse_masked", "attn_merge"):
        assert ops.hip_available(name), (
            f"native _pa_hip extension with {name} must be present")


# every case is built once and never modified
@functools.lru_cache(maxsize=None)
def _random(regime, grid, D, dtype, masked=False):
    case = A.rounding_case(regime, *grid, D, dtype)
    if masked:
        case["keys"] = torch.stack(
            [torch.rand(A.SK, generator=A._gen(90 + b)) < 0.5
             for b in range(grid[0])])
    return case


@functools.lru_cache(maxsize=None)
def _constant(D, dtype):
    return A.constant_columns(*XCD, D, dtype, 3.0)


@functools.lru_cache(maxsize=None)
def _gather(variant, D, dtype):
    return A.one_hot_gather(variant, *XCD, D, dtype)


def _merge(outs, lses, return_lse=False):
    return ops.attention_merge(outs, lses, return_lse)


def _bhsd(t, bshd):
    """A merged result in the call's layout -> [B,H,Sq,...] on the CPU."""
    if bshd:
        t = t.permute(0, 2, 1, 3) if t.dim() == 4 else t.permute(0, 2, 1)
    return t.cpu()


# ------------------------------------------------- the LSE call's two outputs

@pytest.mark.parametrize("masked", [False, True],
                         ids=["unmasked", "bernoulli"])
@pytest.mark.parametrize("route", ["bhsd", "bshd"])
@GRID
@DT
@DIMS
def test_out_is_the_plain_ops(D, dtype, grid, route, masked, no_fallback):
    """The flag adds a store and nothing else: out is torch.equal to
    ops.attention* for the same arguments; lse is fp32, in the output's
    layout without D, and within the bound."""
    case = _random("flat_offset", grid, D, dtype, masked)
    out, lse = L.run_ops_lse(case, route, "cuda")
    assert torch.equal(out, L.run_ops_lse(case, route, "cuda", plain=True))
    L.check_lse(lse, L.lse64(case), f"{route} {grid} D={D} {dtype}")


@pytest.mark.parametrize("scale", A.MODEL_SCALES, ids=["default", "s0.3"])
@pytest.mark.parametrize("regime", A.MODEL_REGIMES)
@GRID
@DT
@DIMS
def test_lse_against_fp64(D, dtype, grid, regime, scale, no_fallback):
    case = _random(regime, grid, D, dtype)
    ref = L.lse64(case, scale)
    for route in ("bhsd", "bshd"):
        _, lse = L.run_ops_lse(case, route, "cuda", scale)
        L.check_lse(lse, ref, f"{regime} {route} {grid} D={D} {dtype} "
                              f"scale={scale}")


@DT
def test_pad_route_and_fused_views(dtype, no_fallback):
    """D = 40 zero-padded to 64 on the BSHD op, and the three strided views
    of one [B, S, 3, H, D] buffer (S = 321), each once."""
    case = _random("flat_offset", XCD, 40, dtype, True)
    out, lse = L.run_ops_lse(case, "bshd", "cuda")
    assert out.shape[-1] == 40
    assert torch.equal(out, L.run_ops_lse(case, "bshd", "cuda", plain=True))
    L.check_lse(lse, L.lse64(case), "pad D=40")
    case = dict(_random("peaked", XCD, 128, dtype))
    case["q"] = torch.cat([case["q"], case["q"][:, :, :A.SK - A.SQ]], 2)
    out, lse = L.run_ops_lse(case, "fused", "cuda")
    assert torch.equal(out, L.run_ops_lse(case, "fused", "cuda", plain=True))
    L.check_lse(lse, L.lse64(case), "fused views")


@BSHD
@DT
@DIMS
def test_rows_without_a_key(D, dtype, bshd, no_fallback):
    """A batch element with no live key (NaN in its K/V) and Sk = 0: lse
    exactly -inf and out exactly +0 on every row. q = 0: lse = log(n)."""
    route = "bshd" if bshd else "bhsd"
    case = L.dead_batch_case(D, dtype)
    ref = L.lse64(dict(case, k=torch.nan_to_num(case["k"])))
    out, lse = L.run_ops_lse(case, route, "cuda")
    L.check_lse(lse, ref, f"dead batch {route}")
    L.check_dead_out(out, ref, f"dead batch {route}")
    empty = dict(case, k=case["k"][:, :, :0], v=case["v"][:, :, :0],
                 keys=None)
    out, lse = L.run_ops_lse(empty, route, "cuda")
    assert (lse == L.NEG_INF).all() and lse.dtype == torch.float32
    A.same_bits(out.cpu(), torch.zeros_like(case["q"]), "Sk = 0")
    zero = dict(case, q=torch.zeros_like(case["q"]))
    want = torch.log(case["keys"].sum(1).double())[:, None, None].expand(
        ref.shape)
    L.check_lse(L.run_ops_lse(zero, route, "cuda")[1], want, "q = 0")
    nokeys = dict(zero, keys=None, k=torch.nan_to_num(case["k"]))
    L.check_lse(L.run_ops_lse(nokeys, route, "cuda")[1],
                torch.full(ref.shape, float(A.SK)).double().log(), "q = 0")


@pytest.mark.parametrize("which", ["B", "H", "Sq"])
def test_empties(which, no_fallback):
    dims = dict(B=2, H=4, Sq=40)
    dims[which] = 0
    q = torch.zeros(dims["B"], dims["Sq"], dims["H"], 64, dtype=C.F16,
                    device="cuda")
    k = torch.zeros(dims["B"], 70, dims["H"], 64, dtype=C.F16, device="cuda")
    out, lse = ops.attention_bshd_lse(q, k, k)
    assert out.shape == q.shape and lse.shape == q.shape[:-1]
    out, lse = ops.attention_lse(*(t.permute(0, 2, 1, 3) for t in (q, k, k)))
    assert lse.shape == (dims["B"], dims["H"], dims["Sq"])
    assert ops.attention_merge([out, out], [lse, lse]).shape == out.shape
    torch.cuda.synchronize()


# ------------------------------------------------------ merge, exact cases

@BSHD
@CUTS
@DT
@DIMS
def test_merge_exact_cases(D, dtype, cuts, bshd, no_fallback):
    """constant_columns cut along the keys: every partial returns the
    constants and the merge returns them bit for bit. one_hot_gather: the
    merged row is v[pi] bit for bit (all but one weight are exactly 0), and
    the merged lse is the unsplit call's within the bound."""
    case = _constant(D, dtype)
    outs, lses = L.chunk_partials(case, L.CUTS[cuts], "cuda", bshd=bshd)
    assert len(outs) == len(L.CUTS[cuts])
    for o in outs:
        A.check_constant(_bhsd(o, bshd), case, "partial")
    L.check_merge_constant(_bhsd(_merge(outs, lses), bshd), case, cuts)
    for variant in ("rising", "dead_twin"):
        case = _gather(variant, D, dtype)
        outs, lses = L.chunk_partials(case, L.CUTS[cuts], "cuda", bshd=bshd)
        out, lse = _merge(outs, lses, return_lse=True)
        L.check_merge_gather(_bhsd(out, bshd), case, f"{variant} {cuts}")
        L.check_lse(_bhsd(lse, bshd), L.lse64(case), f"{variant} {cuts}")


@DT
@DIMS
def test_merge_degenerate_partials(D, dtype, no_fallback):
    """N = 1 is its input bit for bit; a partial with lse = -inf and out =
    NaN changes nothing; all partials -inf give +0 and -inf."""
    case = _random("peaked", XCD, D, dtype)
    outs, lses = L.chunk_partials(case, L.CUTS3, "cuda")
    one = outs[0].clone()
    one.view(torch.int16)[0, 0, 0, :4] = torch.tensor(
        [-32768, 0, 1, -32767], dtype=torch.int16, device="cuda")
    got, lse = _merge([one], [lses[0]], return_lse=True)
    assert torch.equal(A._bits(got), A._bits(one)), "N = 1"
    assert torch.equal(lse, lses[0])
    L.check_merge_skips_dead(_merge, outs, lses, str(dtype))
    dead = [torch.full_like(l, L.NEG_INF) for l in lses]
    nan = [torch.full_like(o, float("nan")) for o in outs]
    out, lse = _merge(nan, dead, return_lse=True)
    A.same_bits(out.cpu(), torch.zeros_like(out).cpu(), "all dead")
    assert (lse == L.NEG_INF).all()


# ---------------------------------------------------- merge, rounding model

@pytest.mark.parametrize("scale", A.MODEL_SCALES, ids=["default", "s0.3"])
@pytest.mark.parametrize("regime", A.MODEL_REGIMES)
@CUTS
@DT
@DIMS
def test_merge_rounding_model(D, dtype, cuts, regime, scale, no_fallback):
    """merge(chunks) against fp64, per element, to the unsplit kernel's bound
    plus half a spacing of each partial times its weight; return_lse against
    the fp64 logsumexp of the unsplit problem."""
    case, r = L.merge_case(regime, XCD, D, dtype, scale, cuts)
    outs, lses = L.chunk_partials(case, L.CUTS[cuts], "cuda", scale)
    out, lse = _merge(outs, lses, return_lse=True)
    what = f"{regime} D={D} {dtype} scale={scale} cuts={cuts}"
    L.check_merge_bound(out.cpu(), r, dtype, what)
    L.check_lse(lse, r["lse"], what)
    _, whole = L.run_ops_lse(case, "bhsd", "cuda", scale)
    L.check_lse(whole, r["lse"], what + " unsplit")


# ---------------------------------------------------------------- refusals

def test_refusals(no_fallback):
    """Each refusal is followed by a valid call, and that call is right."""
    g = torch.Generator(device="cpu").manual_seed(5)
    q, k, v = (torch.randn(2, 300, 4, 64, generator=g).to(C.BF16).cuda()
               for _ in range(3))
    bm = torch.ones(2, 5, dtype=torch.bool, device="cuda")
    with pytest.raises(ValueError, match="block mask"):
        ops.attention_bshd_lse(q, k, v, block_mask=bm)
    with pytest.raises(ValueError, match="block mask"):
        ops.attention_lse(q, k, v, block_mask=bm)
    with pytest.raises(ValueError, match="heads"):
        ops.attention_bshd_lse(q, k[:, :, :3], v[:, :, :3])
    o, l = ops.attention_bshd_lse(q, k, v)
    assert torch.equal(o, ops.attention_bshd(q, k, v))

    def valid():
        out, lse = ops.attention_merge([o, o], [l, l], return_lse=True)
        assert torch.equal(out, o)
        torch.testing.assert_close(lse, l + 0.6931471805599453)

    for n in (0, 9):
        with pytest.raises(ValueError, match="1 to 8"):
            ops.attention_merge([o] * n, [l] * n)
        valid()
    ext = ops.hip_ext()
    bad = {
        "shape": ([o, o[:1]], [l, l[:1]]),
        "lse shape": ([o, o], [l, l[:, :299]]),
        "dtype": ([o, o.half()], [l, l]),
        "bf16 lse": ([o, o], [l, l.bfloat16()]),
        "device": ([o, o.cpu()], [l, l.cpu()]),
    }
    for name, (outs, lses) in bad.items():
        with pytest.raises(RuntimeError):
            ops.attention_merge(outs, lses)
        with pytest.raises(RuntimeError):
            ext.attn_merge(outs, lses, False)
        valid()
    with pytest.raises(RuntimeError, match="1 to 8"):
        ext.attn_merge([o] * 9, [l] * 9, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.attn_merge([o.transpose(1, 2)], [l.transpose(1, 2)], False)
    valid()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the ring

@DT
def test_ring_of_one_rank_is_attention_bshd(dtype, no_fallback):
    from comfyui_parallelanything_amd.parallel.dist import DistInfo
    from comfyui_parallelanything_amd.parallel.sequence import (
        ring_attention_bshd,
    )

    g = torch.Generator(device="cpu").manual_seed(6)
    qkv = torch.randn(2, 300, 3, 4, 128, generator=g).to(dtype).cuda()
    q, k, v = qkv.unbind(2)                     # the fused GEMM's views
    info = DistInfo(0, 1, 0, torch.device("cuda:0"), "nccl")
    out = ring_attention_bshd(q, k, v, None, [300], info)
    assert torch.equal(out, ops.attention_bshd(q, k, v))


def test_two_rank_ring_and_wan():
    """Two processes over RCCL: the ring at S = 600 split 300/300, and tiny
    WAN in bf16, against the single-process result (tests/sp_two_rank_child
    .py compares on every rank)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--standalone",
         "--nproc_per_node", "2",
         os.path.join(root, "tests", "sp_two_rank_child.py")],
        cwd=root, timeout=240)
    assert r.returncode == 0
