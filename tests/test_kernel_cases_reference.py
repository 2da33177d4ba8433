"""The off-N(0,1) kernel cases of kernel_cases.py discriminate (CPU, runs
anywhere).

test_gpu_attn_regimes.py and test_gpu_norm_regimes.py run the native kernels
on these inputs. Here plain-torch emulations of the kernels' arithmetic
stand in for them, at the same shapes and with the same comparison: the
faithful emulation passes every case, every injected fault is rejected by at
least one, and the conditions on the inputs that make it so are asserted on
the reference alone.
"""
import pytest
import torch
import torch.nn.functional as F

import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DIMS = pytest.mark.parametrize("D", C.DIMS)


# ------------------------------------------------------------- attention

def _attention_cases(D, dtype, regimes=("negative_scores", "uniform_ones")):
    """(name, case) for every attention case the GPU file runs at (D,
    dtype)."""
    for regime in regimes:
        for Sk in C.TAIL_SK + (C.CONTROL_SK,):
            for Sq in C.TAIL_SQ:
                yield (f"tail {regime} Sq={Sq} Sk={Sk}",
                       C.tail_case(regime, D, dtype, Sq, Sk))
        for Sk in C.MASK_SK:
            yield f"mask {regime} Sk={Sk}", C.mask_case(regime, D, dtype, Sk)
        if regime == "negative_scores":
            Dp = C.PAD_DIMS[C.DIMS.index(D)]     # the pad route's case
            yield (f"mask {regime} D={Dp} Sk={C.PAD_SK}",
                   C.mask_case(regime, Dp, dtype, C.PAD_SK))
        yield f"block {regime}", C.block_case(regime, D, dtype)


def _staircases(D, dtype):
    for reverse in (False, True):
        for masked in (False, True):
            yield (f"staircase reverse={reverse} masked={masked}",
                   C.staircase_case(D, dtype, reverse, masked))


@pytest.fixture(scope="module")
def cases():
    """{(D, dtype): [(name, case, fp32 reference)]}, computed once."""
    out = {}
    for D in C.DIMS:
        for dtype in C.DTYPES:
            rows = list(_attention_cases(D, dtype)) + list(
                _staircases(D, dtype))
            out[D, dtype] = [(n, c, C.attn_ref(c)) for n, c in rows]
    return out


@DT
@DIMS
def test_faithful_attention_emulation_passes(D, dtype, cases):
    for name, case, ref in cases[D, dtype]:
        out = C.emulate_attention(case)
        assert C.passes(out, ref), f"{name}: max err " \
            f"{(out.float() - ref).abs().max().item():.3g}"
        if "uniform_ones" in name:
            seen = C.visibility(case).any(-1)[:, None, :, None].expand_as(ref)
            assert torch.equal(out.float(), seen.float()), name


def _rejected_by(fault, rows):
    return [n for n, c, ref in rows
            if not C.passes(C.emulate_attention(c, fault=fault), ref)]


@DT
@DIMS
def test_every_sentinel_position_is_rejected_by_negative_scores(D, dtype,
                                                                cases):
    rows = [r for r in cases[D, dtype]
            if "negative_scores" in r[0] and r[1]["keys"] is not None]
    for r in range(C.KV):
        hit = False
        for row in rows:                     # stop at the first rejection
            if _rejected_by(("sentinel", r), [row]):
                hit = True
                break
        assert hit, f"sentinel skipped at bit {r} passes every case"


@DT
@DIMS
def test_every_sentinel_position_is_rejected_by_uniform_ones_exactness(
        D, dtype, cases):
    """The exact-ones criterion of the uniform_ones cases, on its own."""
    rows = [r for r in cases[D, dtype]
            if "mask uniform_ones" in r[0]]
    for r in range(C.KV):
        bad = False
        for name, case, ref in rows:
            out = C.emulate_attention(case, fault=("sentinel", r)).float()
            if not torch.equal(out, ref):
                bad = True
                break
        assert bad, f"sentinel skipped at bit {r} still gives exact ones"


@DT
@DIMS
def test_tail_and_full_and_alpha_faults_are_rejected(D, dtype, cases):
    rows = cases[D, dtype]
    ones_tail = [r for r in rows if r[0].startswith("tail uniform_ones")]
    for d in (1, -1):
        # by the exact-ones criterion the GPU test uses on these cases
        bad = [n for n, c, ref in ones_tail if not torch.equal(
            C.emulate_attention(c, fault=("tail", d)).float(), ref)]
        assert bad, f"tail off by {d} passes every uniform_ones case"
        if d == 1:
            # letting key Sk in shows at every tail length (1 - 1/(Sk+1):
            # 0.5, 0.984, 0.985, 0.995), which only exactness resolves
            assert len(bad) == len(C.TAIL_SK) * len(C.TAIL_SQ), bad
    neg = [r for r in rows if "negative_scores" in r[0]]
    assert _rejected_by(("tail", 1), neg)
    assert _rejected_by(("tail", -1), neg)
    assert _rejected_by(("full",), neg)
    assert _rejected_by(("full",), [r for r in rows if "uniform_ones" in r[0]])
    # the all-full control has nothing a tail or full fault could change
    control = [r for r in rows if f"Sk={C.CONTROL_SK}" in r[0]]
    for fault in (("tail", 1), ("full",), ("sentinel", 5)):
        assert not _rejected_by(fault, control)
    stairs = [r for r in rows if r[0].startswith("staircase")]
    bad = _rejected_by(("alpha", 1), stairs)
    assert any("reverse=False" in n for n in bad)


@DT
@DIMS
def test_negative_scores_make_a_phantom_key_heavy(D, dtype, cases):
    """w = 1 / (1 + sum of exp(visible scores)) >= 0.25 on every row that
    sees a key, and an output shrunk by that weight (what one zero-V phantom
    does) fails the comparison."""
    for name, case, ref in cases[D, dtype]:
        if "negative_scores" not in name:
            continue
        w = C.phantom_weight(case)
        seen = C.visibility(case).any(-1)[:, None, :].expand_as(w)
        assert w[seen].min().item() >= 0.25, f"{name}: {w[seen].min()}"
        shrunk = ref * (1.0 - w.float())[..., None]
        assert not C.passes(shrunk, ref), name


@DIMS
def test_masks_cover_every_bit_position(D):
    """Over the processed partial tiles of each masked case, every bit
    position 0..63 is dead at least once and live at least once."""
    for regime in ("negative_scores",):
        for name, case in _attention_cases(D, C.BF16, (regime,)):
            if case["keys"] is None:
                continue
            dead = torch.zeros(C.KV, dtype=torch.bool)
            live = torch.zeros(C.KV, dtype=torch.bool)
            for b, qb, t, bits in C.processed_tiles(case):
                if not bits.all():
                    dead |= ~bits
                    live |= bits
            assert dead.all(), f"{name}: never dead {(~dead).nonzero().T}"
            assert live.all(), f"{name}: never live {(~live).nonzero().T}"


@pytest.mark.parametrize("scale", [-0.125, 0.0, float("nan")])
def test_nonpositive_scale_is_refused_on_every_device(scale):
    """The native kernels need scale > 0 (raw-score maximum, negative
    sentinel); ops refuses the rest on the CPU too, so both paths take the
    same arguments."""
    case = C.tail_case("negative_scores", 64, torch.float32, 5, 9)
    q, k, v = case["q"], case["k"], case["v"]
    qs, ks, vs = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    with pytest.raises(ValueError, match="scale"):
        ops.attention(q, k, v, scale)
    with pytest.raises(ValueError, match="scale"):
        ops.attention_bshd(qs, ks, vs, scale)
    with pytest.raises(ValueError, match="scale"):
        ops.attention_bshd_split(qs, ks, vs, 2, scale)
    assert torch.equal(ops.attention(q, k, v, 0.125),
                       R.attention(q, k, v, 0.125))


def test_block_case_has_uneven_lists_and_blind_rows():
    case = C.block_case("uniform_ones", 64, C.BF16)
    per = {}
    for b, qb, t, bits in C.processed_tiles(case):
        per[b, qb] = per.get((b, qb), 0) + 1
    assert len(set(per.values())) > 1
    blind = ~C.visibility(case).any(-1)
    assert blind.any() and not blind.all()


def test_staircase_drives_both_alpha_paths():
    """Forward: most rows raise their maximum on every tile. Reversed: most
    rows never raise it after the first."""
    for reverse, want_growth in ((False, True), (True, False)):
        case = C.staircase_case(128, C.BF16, reverse, False)
        s = torch.matmul(case["q"].float(),
                         case["k"].float().transpose(-1, -2))
        tmax = s.view(*s.shape[:-1], -1, C.KV).amax(-1)       # per tile
        run = torch.cummax(tmax, -1).values
        grew = (run[..., 1:] > run[..., :-1]).float().mean().item()
        assert (grew > 0.8) if want_growth else (grew < 0.2), grew


# ------------------------------------------------------------------ norms

def _ln_inputs(dtype, vec=8):
    """(name, x [rows, D], eps) of every LayerNorm row the GPU file runs on
    the vector kernels (vec=8) or the scalar ones (vec=1)."""
    for D in C.LN_DIMS:
        if D % vec:
            continue
        for regime, eps in C.NORM_RUNS:
            rows = C.CONSTANT_ROWS if regime == "constant" else 6
            yield (f"{regime} D={D} eps={eps}",
                   C.norm_rows(regime, rows, D, dtype, D), eps)


@DT
@pytest.mark.parametrize("fused", [True, False], ids=["fma", "mul_add"])
def test_faithful_norm_emulation_passes(dtype, fused):
    for name, x, eps in _ln_inputs(dtype):
        out = C.emulate_layer_norm(x, eps, fused=fused)
        assert torch.isfinite(out.float()).all(), name
        assert C.passes(out, C.layer_norm_f64(x, eps), *C.TOL_LN), name


@DT
@pytest.mark.parametrize("fault", C.NORM_FAULTS)
def test_every_norm_fault_is_rejected(dtype, fault):
    """Under at least one of the two rounding models for x*x + s2; the
    unclamped variance is the one whose sign depends on the model."""
    bad = []
    for name, x, eps in _ln_inputs(dtype):
        for fused in (True, False):
            out = C.emulate_layer_norm(x, eps, fault=fault, fused=fused)
            if not C.passes(out, C.layer_norm_f64(x, eps), *C.TOL_LN):
                bad.append(name)
    if fault == "no_clamp" and dtype == C.BF16:
        # the emulation finds no negative variance for a bf16 constant (8
        # significant bits: n * c * c stays exact far longer)
        return
    assert bad, f"{fault} passes every case"
    want = {"no_eps": "tiny", "eps_outside": "tiny", "no_mean": "offset",
            "no_clamp": "constant", "skip_last": "outlier"}[fault]
    hit = {n for n in bad if n.startswith(want)}
    if fault == "no_clamp":
        assert hit, bad
    else:
        # at every width and eps the regime runs at, not only where randn
        # would do (the mean of 8 draws is 0.35, of 5120 it is 0.014)
        every = {n for n, _, _ in _ln_inputs(dtype) if n.startswith(want)}
        assert hit == every, sorted(every - hit)


@DT
def test_huge_rows_reach_the_top_of_the_format(dtype):
    """Every element is at the magnitude where a 16-bit or unscaled sum
    would overflow, and the fp32 sum of squares still fits."""
    for D in C.LN_DIMS:
        x = C.huge(6, D, dtype, D).float()
        assert x.abs().min() >= (3e4 if dtype == C.F16 else 9e14)
        assert (x > 0).any() and (x < 0).any()
        assert x.pow(2).sum(-1).max() < 1e38
        out = C.emulate_layer_norm(C.huge(6, D, dtype, D),
                                   vec=1 if D % 8 else 8)
        assert torch.isfinite(out.float()).all()


def test_unclamped_variance_goes_negative_on_fp16_constants():
    """The hazard the clamp removes, on the emulation: at WAN's and FLUX's
    widths some fp16 constant rows have E[x^2] - mean^2 < 0 and come out
    NaN without the clamp, finite with it."""
    for D in (3072, 5120):
        x = C.constant(C.CONSTANT_ROWS, D, C.F16)
        nan_rows = set()
        for fused in (True, False):
            out = C.emulate_layer_norm(x, fault="no_clamp", fused=fused)
            nan_rows |= set(out.float().isnan().any(-1).nonzero()
                            .flatten().tolist())
            ok = C.emulate_layer_norm(x, fused=fused)
            assert torch.equal(ok.float(), torch.zeros_like(ok.float()))
        assert nan_rows, f"D={D}: no constant gives a negative variance"


def test_fp32_rows_need_the_deviation_pass():
    """fp32 inputs are held to 1e-5. Emulated, the single-pass variance
    misses that on offset rows (4e-4 off at mean 40) and nowhere else but
    on constant rows, whose mean fp32 cannot hold; with the pass over the
    deviations every regime but those constants is inside."""
    f32 = torch.float32
    missed = set()
    for name, x, eps in _ln_inputs(f32, vec=1):
        ref = C.layer_norm_f64(x, eps)
        one = C.emulate_layer_norm(x, eps, vec=1)
        two = C.emulate_layer_norm(x, eps, vec=1, deviation_pass=True)
        assert torch.isfinite(two).all(), name
        if not C.passes(one, ref, *C.TOL_FP32):
            missed.add(name.split()[0])
        if not name.startswith("constant"):
            assert C.passes(two, ref, *C.TOL_FP32), name
    assert "offset" in missed and missed <= {"offset", "constant"}, missed


def _ref_close(ref32, ref64, tol, part=4):
    """The fp32 reference within a quarter of the tolerance of fp64."""
    return C.passes(ref32, ref64, tol[0] / part, tol[1] / part)


def _norm_reference_cases(dtype):
    """(what, op, regime, fp32 reference rows, fp64 rows, tolerance) for
    every norm case of the GPU file."""
    for regime, eps in C.NORM_RUNS:
        n = C.CONSTANT_ROWS if regime == "constant" else 6
        for _, D in C.RMS_SHAPES + tuple((9, d) for d in C.QK_DIMS):
            x = C.norm_rows(regime, n, D, dtype, D)
            w = C.plain(1, D, dtype, 5)[0]
            yield (f"rms_norm {regime} D={D} eps={eps}", "rms_norm",
                   regime, R.rms_norm(x.float(), w.float(), eps),
                   C.rms_norm_f64(x, w, eps), C.norm_tol(dtype, C.TOL_RMS))
        for D in C.LN_DIMS:
            x = C.norm_rows(regime, n, D, dtype, D).view(2, n // 2, D)
            sc, sh = C.modulation(2, D, dtype, 6)
            yield (f"layer_norm_mod {regime} D={D} eps={eps}",
                   "layer_norm_mod", regime,
                   R.layer_norm_mod(x.float(), sc.float(), sh.float(),
                                    eps).view(n, D),
                   C.layer_norm_mod_f64(x, sc, sh, eps).view(n, D),
                   C.norm_tol(dtype, C.TOL_LN))
        for shape in C.GN_SHAPES:
            x, w, b, G = C.group_norm_case(regime, shape, dtype)
            rows = x.shape[0] * G
            yield (f"group_norm_silu {regime} {shape} eps={eps}",
                   "group_norm_silu", regime,
                   R.group_norm_silu(x.float(), G, w.float(), b.float(),
                                     eps).reshape(rows, -1),
                   C.group_norm_silu_f64(x, G, w, b, eps).reshape(rows, -1),
                   C.norm_tol(dtype, C.TOL_GN))


@pytest.mark.parametrize("dtype", C.DTYPES + (torch.float32,),
                         ids=C.DTYPE_IDS + ("fp32",))
def test_references_agree_with_fp64(dtype):
    """ops.reference (fp32, two-pass: F.layer_norm, F.group_norm) against the
    inline fp64 formulas on every norm case, within a quarter of the op's
    tolerance (fp32 inputs: within the tolerance, and see below for offset
    rows). Constant rows go one at
    a time: every constant the GPU tests compare for closeness is close
    here, every 16-bit constant they only check for finiteness is far
    somewhere, and those are at most half."""
    f32 = dtype == torch.float32
    far = {op: set() for op in C.FINITE_ONLY_CONSTANTS}
    for what, op, regime, r32, r64, tol in _norm_reference_cases(dtype):
        if regime != "constant":
            if f32 and regime == "offset":
                # uncompensated fp32 cannot hold a mean of 40 closer than
                # half an ulp, 1.9e-6, and sums it about as well; times
                # 1 + scale (up to 5) that is 2e-5 on top of the 1e-5. The
                # kernels carry the mean's remainder and are held to 1e-5.
                tol = (tol[0], tol[1] + 2e-5)
            assert _ref_close(r32, r64, tol, 1 if f32 else 4), what
            continue
        for i in range(r32.shape[0]):
            if _ref_close(r32[i], r64[i], tol):
                continue
            c = C.CONSTANTS[i % len(C.CONSTANTS)]
            assert not C.compared_constant(op, dtype, i), \
                f"{what}: constant {c} is compared but far from fp64"
            far[op].add(c)
    for op, listed in C.FINITE_ONLY_CONSTANTS.items():
        assert len(listed) <= len(C.CONSTANTS) // 2
        if dtype == C.BF16:
            assert far[op] == set(listed), (op, far[op])


def test_gelu_values_are_what_the_kernel_must_survive():
    for dtype in C.DTYPES:
        x = C.gelu_values(dtype)
        assert x.numel() % 8 == 0
        assert x.isnan().sum() == 1 and x.isinf().sum() == 2
        ref = F.gelu(x.float(), approximate="tanh")
        # saturated ends: identity and (signed) zero, no NaN but NaN's own
        # and -inf's (0 * inf)
        assert ref.isnan().sum() == 2
        big = x.float() >= 20
        assert torch.equal(ref[big], x.float()[big])
