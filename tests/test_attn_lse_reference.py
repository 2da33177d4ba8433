"""attn_lse_cases.py proves itself on the CPU: the faithful emulation of the
LSE epilogue and of the merge kernel, and ops.* on the reference path, pass
every check; each injected fault is rejected by the check named beside it.
test_gpu_attn_lse.py runs the native kernels through the same checks.
"""
import functools

import pytest
import torch

import attention_cases as A
import attn_lse_cases as L
import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DIMS = pytest.mark.parametrize("D", C.DIMS)
CUTS = pytest.mark.parametrize("cuts", ["3", "8"])
XCD = A.GRIDS[0]


def _model_keys(grids=A.GRIDS):
    return [(regime, grid, D, dtype, scale)
            for regime in A.MODEL_REGIMES for grid in grids for D in C.DIMS
            for dtype in C.DTYPES for scale in A.MODEL_SCALES]


@functools.lru_cache(maxsize=None)
def _case(regime, grid, D, dtype):
    return A.rounding_case(regime, *grid, D, dtype)


# ------------------------------------------------------------------ the lse

def test_lse_bound_is_twice_the_measured_worst():
    """The fp32 emulation against fp64 in units of 2^-21 + 2^-24 |lse|, over
    every case the GPU file uses; every case within the bound."""
    worst = 0.0
    for regime, grid, D, dtype, scale in _model_keys():
        case = _case(regime, grid, D, dtype)
        ref = L.lse64(case, scale)
        lse = L.emulate_lse(case, scale)
        worst = max(worst, L.lse_distance(lse, ref))
        L.check_lse(lse, ref, f"{regime} {grid} D={D} {dtype} {scale}")
    assert 0.8 * L.LSE_MEASURED <= worst <= L.LSE_MEASURED, worst
    assert L.LSE_A == 2 * L.LSE_MEASURED * 2.0 ** -21
    assert L.LSE_B == 2 * L.LSE_MEASURED * 2.0 ** -24


@pytest.mark.parametrize("route", L.LSE_ROUTES)
@DT
def test_ops_on_cpu_pass_the_lse_checks(dtype, route):
    """ops.attention_lse / attention_bshd_lse on the reference path: the out
    of the plain op bit for bit, the lse within the bound, in the output's
    layout without D."""
    for regime in A.MODEL_REGIMES:
        case = dict(_case(regime, XCD, 64, dtype))
        if route == "fused":
            case["q"] = torch.cat([case["q"], case["q"][:, :, :21]], 2)
        out, lse = L.run_ops_lse(case, route)
        assert torch.equal(out, L.run_ops_lse(case, route, plain=True))
        L.check_lse(lse, L.lse64(case), f"cpu {route} {regime}")


@DT
def test_dead_rows_are_minus_inf_and_zero(dtype):
    """A batch element with no live key (its K/V NaN), and Sk = 0: lse -inf,
    out +0, from the emulation and from the ops; q = 0: lse = log(n_visible)."""
    case = L.dead_batch_case(64, dtype)
    ref = L.lse64(dict(case, k=torch.nan_to_num(case["k"])))
    assert (ref[1] == L.NEG_INF).all() and torch.isfinite(ref[0]).all()
    L.check_lse(L.emulate_lse(case), ref, "emulation")
    for route in ("bhsd", "bshd"):
        out, lse = L.run_ops_lse(case, route)
        L.check_lse(lse, ref, f"cpu {route}")
        L.check_dead_out(out, ref, f"cpu {route}")
    q = case["q"]
    empty = q[:, :, :0]
    out, lse = ops.attention_lse(q, empty, empty)
    assert (lse == L.NEG_INF).all() and lse.shape == q.shape[:-1]
    A.same_bits(out, torch.zeros_like(q), "Sk = 0")
    zero = dict(case, q=torch.zeros_like(q))
    n = case["keys"].sum(1).double()
    want = torch.log(n)[:, None, None].expand(ref.shape)
    L.check_lse(L.emulate_lse(zero), want, "q = 0, emulation")
    L.check_lse(L.run_ops_lse(zero)[1], want, "q = 0, cpu")


@pytest.mark.parametrize("which", ["B", "H", "Sq"])
def test_empties(which):
    dims = dict(B=2, H=3, Sq=5)
    dims[which] = 0
    q = torch.randn(dims["B"], dims["H"], dims["Sq"], 16)
    k = torch.randn(dims["B"], dims["H"], 7, 16)
    out, lse = ops.attention_lse(q, k, k)
    assert out.shape == q.shape and lse.shape == q.shape[:-1]
    out, lse = ops.attention_bshd_lse(*(t.permute(0, 2, 1, 3)
                                        for t in (q, k, k)))
    assert lse.shape == (dims["B"], dims["Sq"], dims["H"])


LSE_REJECTED_BY = {
    "log2_domain": "lse_bound", "no_log_l": "lse_bound",
    "first_tile": "lse_bound", "sentinel": "lse_dead_rows",
    "bhswap": "lse_bound", "bhs_on_bshd": "lse_bound",
}


@pytest.mark.parametrize("fault", L.LSE_FAULTS)
@DT
def test_lse_faults_are_rejected(dtype, fault):
    assert set(LSE_REJECTED_BY) == set(L.LSE_FAULTS)
    if fault == "sentinel":
        case = L.dead_batch_case(64, dtype)
        ref = L.lse64(dict(case, k=torch.nan_to_num(case["k"])))
    else:
        case = _case("flat_offset", XCD, 64, dtype)
        ref = L.lse64(case)
    bshd = fault == "bhs_on_bshd"
    good = L.emulate_lse(case, bshd=bshd)
    bad = L.emulate_lse(case, fault=fault, bshd=bshd)
    if bshd:
        good, bad = good.permute(0, 2, 1), bad.permute(0, 2, 1)
    L.check_lse(good, ref, "faithful")
    with pytest.raises(AssertionError, match=LSE_REJECTED_BY[fault]):
        L.check_lse(bad, ref, fault)


def test_block_mask_is_refused():
    q = torch.randn(1, 2, 300, 16)
    bm = torch.ones(2, 5, dtype=torch.bool)
    with pytest.raises(ValueError, match="block mask"):
        ops.attention_lse(q, q, q, block_mask=bm)
    with pytest.raises(ValueError, match="block mask"):
        ops.attention_bshd_lse(q, q, q, block_mask=bm)
    assert torch.isfinite(ops.attention_lse(q, q, q)[1]).all()


# ---------------------------------------------------------------- the merge

@functools.lru_cache(maxsize=None)
def _constant(dtype):
    return A.constant_columns(*XCD, 64, dtype, 3.0)


@functools.lru_cache(maxsize=None)
def _gather(variant, dtype):
    return A.one_hot_gather(variant, *XCD, 64, dtype)


def _cpu_merge(outs, lses, return_lse=False):
    return ops.attention_merge(outs, lses, return_lse)


MERGES = pytest.mark.parametrize(
    "merge", [L.emulate_merge, _cpu_merge], ids=["emulation", "ops_cpu"])


@MERGES
@CUTS
@DT
def test_merge_exact_cases(dtype, cuts, merge):
    """constant_columns: every partial returns the constants, the merge
    returns them. one_hot_gather: the merged row is v[pi]; all but one
    weight are exactly 0. Partials from the emulation."""
    case = _constant(dtype)
    outs, lses = L.emulated_partials(case, L.CUTS[cuts])
    for o in outs:
        A.check_constant(o, case, "partial")
    L.check_merge_constant(merge(outs, lses), case, cuts)
    for variant in ("rising", "dead_twin"):
        case = _gather(variant, dtype)
        outs, lses = L.emulated_partials(case, L.CUTS[cuts])
        out, lse = merge(outs, lses, return_lse=True)
        L.check_merge_gather(out, case, f"{variant} {cuts}")
        L.check_lse(lse, L.lse64(case), f"{variant} {cuts} merged lse")


@MERGES
@DT
def test_merge_degenerate_partials(dtype, merge):
    """N = 1 bit for bit (-0.0 and NaN included); a dead partial with NaN
    changes nothing; all dead gives +0 and -inf."""
    case = _case("peaked", XCD, 64, dtype)
    outs, lses = L.emulated_partials(case, L.CUTS3)
    one = outs[0].clone()
    one.view(torch.int16)[0, 0, 0, :4] = torch.tensor(
        [-32768, 0, 1, -32767], dtype=torch.int16)      # -0, +0, subnormals
    got = merge([one], [lses[0]])
    assert torch.equal(A._bits(got), A._bits(one)), "N = 1"
    L.check_merge_skips_dead(merge, outs, lses, str(dtype))
    dead = [torch.full_like(l, L.NEG_INF) for l in lses]
    nan = [torch.full_like(o, float("nan")) for o in outs]
    out, lse = merge(nan, dead, return_lse=True)
    A.same_bits(out, torch.zeros_like(out), "all dead")
    assert (lse == L.NEG_INF).all()


@CUTS
@DT
def test_merge_bound_holds_the_emulation_not_pairwise(dtype, cuts):
    """D = 64: the emulation stays under 1.0 of the merge bound in every
    regime at both scales; partials folded pairwise with a 16-bit rounding
    between folds do not (at eight chunks: seven roundings). The merged lse
    equals the unsplit lse within the lse bound."""
    worst_old = pairwise = 0.0
    for regime in A.MODEL_REGIMES:
        for scale in A.MODEL_SCALES:
            case, r = L.merge_case(regime, XCD, 64, dtype, scale, cuts)
            outs, lses = L.emulated_partials(case, L.CUTS[cuts], scale)
            out, lse = L.emulate_merge(outs, lses, return_lse=True)
            what = f"{regime} {scale} {cuts}"
            L.check_merge_bound(out, r, dtype, what)
            L.check_lse(lse, r["lse"], what)
            L.check_merge_bound(_cpu_merge(outs, lses), r, dtype,
                                what + " ops_cpu")
            worst_old = max(worst_old, L.merge_distance(out, r, dtype, True))
            pairwise = max(pairwise, L.merge_distance(
                L.emulate_merge(outs, lses, fault="pairwise16"), r, dtype))
    print(f"{dtype} {cuts}: old bound {worst_old:.3f}, pairwise {pairwise:.3f}")
    if cuts == "3":
        assert worst_old > 1.0, "the extra term was needed here"
    else:
        assert pairwise > 1.0


MERGE_REJECTED_BY = {
    "nomax": "merge_gather", "nonorm": "merge_constant",
    "mul_dead": "merge_skips_dead", "pairwise16": "merge_bound",
    "skip_last": "merge_gather",
}


@pytest.mark.parametrize("fault", L.MERGE_FAULTS)
@DT
def test_merge_faults_are_rejected(dtype, fault):
    assert set(MERGE_REJECTED_BY) == set(L.MERGE_FAULTS)

    def bad(outs, lses, return_lse=False):
        return L.emulate_merge(outs, lses, fault, return_lse)

    name = MERGE_REJECTED_BY[fault]
    with pytest.raises(AssertionError, match=name):
        if fault in ("nomax", "skip_last"):
            # scores of 512: exp(lse) overflows without the maximum; rising
            # rows select keys of the last chunk
            case = _gather("rising", dtype)
            outs, lses = L.emulated_partials(case, L.CUTS3)
            L.check_merge_gather(bad(outs, lses), case, fault)
        elif fault == "nonorm":
            case = _constant(dtype)
            outs, lses = L.emulated_partials(case, L.CUTS3)
            L.check_merge_constant(bad(outs, lses), case, fault)
        elif fault == "mul_dead":
            case = _case("peaked", XCD, 64, dtype)
            outs, lses = L.emulated_partials(case, L.CUTS3)
            L.check_merge_skips_dead(bad, outs, lses, fault)
        else:
            case, r = L.merge_case("peaked", XCD, 64, dtype, None, "8")
            outs, lses = L.emulated_partials(case, L.CUTS8)
            L.check_merge_bound(bad(outs, lses), r, dtype, fault)


def test_merge_refusals_on_cpu():
    o = torch.randn(2, 5, 3, 16)
    l = torch.randn(2, 5, 3)
    for n in (0, 9):
        with pytest.raises(ValueError, match="1 to 8"):
            ops.attention_merge([o] * n, [l] * n)
    with pytest.raises(RuntimeError, match="shape"):
        ops.attention_merge([o, o[:1]], [l, l[:1]])
    with pytest.raises(RuntimeError, match="shape"):
        ops.attention_merge([o, o], [l, l[:, :4]])
    with pytest.raises(RuntimeError, match="dtype"):
        ops.attention_merge([o, o.half()], [l, l])
    with pytest.raises(RuntimeError, match="fp32"):
        ops.attention_merge([o, o], [l, l.bfloat16()])
    with pytest.raises(RuntimeError, match="is on"):
        ops.attention_merge([o, o.to("meta")], [l, l])
    out, lse = ops.attention_merge([o, o], [l, l], return_lse=True)
    torch.testing.assert_close(out, o)
    torch.testing.assert_close(lse, l + 0.6931471805599453)
    assert R.MERGE_MAX == ops.ATTN_MERGE_MAX == 8
