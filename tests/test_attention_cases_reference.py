"""The attention cases of attention_cases.py discriminate (CPU, runs
anywhere).

test_gpu_attn_exact.py runs the native kernels through constant_columns,
one_hot_gather and rounding_model. Here a plain-torch emulation of the
kernel's arithmetic stands in for them, at the same shapes and with the same
comparison functions: the faithful emulation passes every check, each
arithmetic fault is rejected by the check named beside it, and the
conditions on the inputs that make it so are asserted on the fp64 reference
alone.

ops.attention* on the CPU (ops.reference: fp32 softmax, P not rounded to 16
bit) is held to every one of the checks too: check_constant, check_gather,
and check_model with the limits of the emulation, through every route.
"""
import pytest
import torch

import attention_cases as A
import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DIMS = pytest.mark.parametrize("D", C.DIMS)
GRID = pytest.mark.parametrize("grid", A.GRIDS, ids=A.GRID_IDS)
XCD = A.GRIDS[0]


def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------ a. constant_columns

def _constant_cases(D, dtype):
    for grid in A.GRIDS:
        for qmul in A.Q_SCALES:
            for mask in (None, "keys"):
                yield (f"{grid} q*{qmul} {mask}",
                       A.constant_columns(*grid, D, dtype, qmul, mask=mask))
    for qmul in A.Q_SCALES:
        yield (f"block q*{qmul}",
               A.constant_columns(0, 0, D, dtype, qmul, mask="block"))
    yield ("fused", A.constant_columns(*XCD, D, dtype, 3.0, Sq=A.FUSED_S,
                                       mask="keys"))


@DT
@DIMS
def test_emulation_returns_the_constants_bit_for_bit(D, dtype):
    for name, case in _constant_cases(D, dtype):
        A.check_constant(A.emulate(case), case, name)
        if case["keys"] is not None:
            blind = ~C.visibility(case).any(-1)
            if "block" in name:
                assert blind.any()           # rows that must be exactly +0
            assert (case["want"][blind[:, None].expand(
                case["want"].shape[:3])] == 0).all()


# check_constant is the check that rejects each of these
CONSTANT_FAULTS = ("trunc", "o16", "l_first", "noxor", "bhswap")


@pytest.mark.parametrize("fault", CONSTANT_FAULTS)
@DT
@DIMS
def test_constant_columns_reject(D, dtype, fault):
    """On every scale of q, masked or not. trunc on 1614 to 2400 of the 2400
    rows, o16 on 2315 to 2400."""
    for qmul in A.Q_SCALES:
        for mask in (None, "keys"):
            case = A.constant_columns(*XCD, D, dtype, qmul, mask=mask)
            out = A.emulate(case, fault=fault)
            assert _rejects(A.check_constant, out, case), (fault, qmul, mask)
            rows = (A._bits(out) != A._bits(case["want"])).any(-1).sum()
            assert rows >= 0.25 * out[..., 0].numel(), (fault, int(rows))


@DT
@DIMS
def test_uniform_ones_cannot_see_truncation(D, dtype):
    """q = 0, v = 1 (kernel_cases.uniform_ones): every P is exactly 1.0 and
    truncation changes nothing, so the old exact case passes a kernel that
    truncates P; the constants on randn scores do not."""
    for mask in (None, "keys"):
        old = A.constant_columns(*XCD, D, dtype, mask=mask, ones=True)
        A.check_constant(A.emulate(old, fault="trunc"), old)
        new = A.constant_columns(*XCD, D, dtype, mask=mask)
        assert _rejects(A.check_constant, A.emulate(new, fault="trunc"), new)


@DIMS
def test_constant_columns_input_conditions(D):
    """No two (b, h) share a column pattern; the list holds the constants
    the contract names; 1 / sum P^2 is about 129 keys on randn scores (every
    row above 10) and about 7.5 with q * 3 (some rows down to one key)."""
    for dtype in C.DTYPES:
        c = A.column_constants(*XCD, D, dtype).reshape(-1, D)
        assert len({tuple(r.tolist()) for r in c}) == c.shape[0]
    for c in (1.0, -1.5, 1.9921875, 2.0 ** -10, 0.3, -7.77, 255.0, 3e4):
        assert c in A.CONSTANTS
    n1 = A.effective_keys(A.constant_columns(*XCD, D, C.BF16, 1.0))
    n3 = A.effective_keys(A.constant_columns(*XCD, D, C.BF16, 3.0))
    assert n1.min() > 10 and 100 < n1.median() < 160
    assert n3.min() < 1.1 and 5 < n3.median() < 10


# -------------------------------------------------------- b. one_hot_gather

@pytest.mark.parametrize("variant", A.GATHER_VARIANTS)
@DT
@DIMS
def test_emulation_gathers_bit_for_bit(D, dtype, variant):
    for grid in A.GRIDS:
        case = A.one_hot_gather(variant, *grid, D, dtype)
        seen = A.check_gather(A.emulate(case), case, f"{variant} {grid}")
        # fp32 arithmetic keeps a subnormal of V; a -0 gains the +0 products
        # of the other keys and comes back +0
        assert seen["subnormal_flushed"] == 0 and seen["neg_zero_kept"] == 0
        if variant in ("rising", "falling") and grid == XCD:
            assert seen["subnormal_kept"] > 0 and seen["neg_zero_lost"] > 0


# check_gather is the check that rejects each of these
GATHER_FAULTS = ("nomax", "vrot8", "noxor", "bhswap", "l_first")


@pytest.mark.parametrize("fault", GATHER_FAULTS)
@DT
@DIMS
def test_one_hot_gather_rejects(D, dtype, fault):
    for variant in ("rising", "falling", "dead_twin"):
        case = A.one_hot_gather(variant, *XCD, D, dtype)
        out = A.emulate(case, fault=fault)
        if fault == "l_first" and variant == "falling":
            continue            # rows whose key is in tile 0 keep l = 1
        assert _rejects(A.check_gather, out, case), (fault, variant)
        if fault == "nomax":
            assert not torch.isfinite(out.float()).all()   # it overflows


@pytest.mark.parametrize("D", C.DIMS + C.PAD_DIMS)
def test_gather_gap_exceeds_160_bits(D):
    """On the fp64 scores alone: the selected key outranks every other
    visible key by MIN_GAP in log2 units, so every other exp2 is exactly 0 in
    fp32 whatever v_exp_f32 does below 2^-149. D = 40 is the tight one: with
    |q| = 64 its gap is 146, hence QMUL[40] = 128."""
    for variant in A.GATHER_VARIANTS:
        for grid in A.GRIDS:
            case = A.one_hot_gather(variant, *grid, D, C.BF16)
            gap = A.gather_gap(case)
            assert gap >= A.MIN_GAP, (variant, grid, gap)
            for dtype in C.DTYPES:           # +-1 and +-QMUL are exact
                c16 = A.one_hot_gather(variant, *grid, D, dtype)
                assert torch.equal(c16["q"].float(), case["q"].float())
                assert torch.equal(c16["k"].float(), case["k"].float())
    if D == 40:
        weak = A.one_hot_gather("rising", *XCD, D, C.BF16)
        weak["q"] = (weak["q"].float() / 2).to(C.BF16)     # |q| = 64
        assert A.gather_gap(weak) < A.MIN_GAP


def test_gather_hits_every_tile_position():
    """Rising and falling: all 64 positions of full tile 1 and the one key
    of the tail tile. dead_twin: every live key of every (partial) tile, which
    in tiles 3 and 4 together is every position 0..63; every dead key has a
    live twin with another V row."""
    for variant in ("rising", "falling"):
        pi = A.one_hot_gather(variant, *XCD, 64, C.BF16)["pi"][0]
        hit = set(pi.tolist())
        assert set(range(64, 128)) <= hit and A.SK - 1 in hit
        assert (pi.diff() > 0).all() or (pi.diff() < 0).all()
        assert len({int(j) // 64 for j in pi}) == 6
    case = A.one_hot_gather("dead_twin", *XCD, 64, C.BF16)
    for b in range(XCD[0]):
        live = case["keys"][b].nonzero().flatten().tolist()
        assert set(case["pi"][b].tolist()) == set(live)
        assert {j % 64 for j in live if j // 64 in (3, 4)} == set(range(64))
        for j in (~case["keys"][b]).nonzero().flatten().tolist():
            twin = [i for i in live
                    if torch.equal(case["k"][b, :, i], case["k"][b, :, j])]
            assert twin and not torch.equal(case["v"][b, :, twin[0]],
                                            case["v"][b, :, j])
    for b, qb, t, bits in C.processed_tiles(case):
        assert not bits.all()                # every processed tile partial
    pair = A.one_hot_gather("pair", *XCD, 64, C.BF16)
    assert torch.equal(pair["k"][:, :, :128], pair["k"][:, :, 128:256])
    assert not torch.equal(pair["v"][:, :, :128], pair["v"][:, :, 128:256])


@DT
@DIMS
def test_gather_holds_every_finite_pattern(D, dtype):
    """V of the rising case at B, H = 2, 4 holds every finite 16-bit pattern,
    and every one of them is the expected output of some row."""
    case = A.one_hot_gather("rising", *XCD, D, dtype)
    fin, huge = A.finite_patterns(dtype)
    want = set(torch.cat([fin, huge]).tolist())
    assert len(want) == 65536 - (256 if dtype == C.BF16 else 2048)
    have_v = set((A._bits(case["v"]).to(torch.int32) & 0xffff).unique()
                 .tolist())
    have_out = set((A._bits(case["want"]).to(torch.int32) & 0xffff).unique()
                   .tolist())
    assert have_v == want and have_out == want
    assert torch.isfinite(case["v"].float()).all()
    if dtype == C.BF16:       # the overflow hazard sits in the last key only
        assert (case["v"][:, :, :-1].float().abs() < 2.0 ** 126).all()


# -------------------------------------------------------- c. rounding_model

def _model_cases(grids=A.GRIDS):
    for grid in grids:
        for D in C.DIMS:
            for dtype in C.DTYPES:
                for regime in A.MODEL_REGIMES:
                    for scale in A.MODEL_SCALES:
                        yield regime, grid, D, dtype, scale


def test_emulation_passes_the_rounding_model():
    """rho is about 1 (0.82 to 1.01) and no element beyond 0.9 of its
    bound; an exp2 and a reciprocal one ulp either way, and P.V summed in the
    reverse order, move rho by less than 1%, where the margin allows 15%."""
    for key in _model_cases():
        case, r, rho = A.model_case(*key)
        scale, dtype = key[4], key[3]
        assert 0.8 < rho < 1.02, (key, rho)
        _, worst = A.check_model(A.emulate(case, scale), r, dtype,
                                 A.RHO_MARGIN * rho, str(key))
        assert worst < 0.9, (key, worst)
        if key[1] != XCD:
            continue
        for kw in (dict(nudge=1), dict(nudge=-1), dict(flip=True)):
            moved, _ = A.check_model(A.emulate(case, scale, **kw), r, dtype,
                                     A.RHO_MARGIN * rho, f"{key} {kw}")
            assert abs(moved / rho - 1) < 0.01, (key, kw, moved, rho)


# regimes in which rho alone (check_model's first assertion) rejects the
# fault, and the smallest rho / emulation's rho there must reach
RHO_REJECTS = {"trunc": (A.MODEL_REGIMES, 1.6),
               "o16": (A.MODEL_REGIMES, 1.6),
               "scale16": (("peaked",), 1.25),
               "qscale16": (("peaked",), 2.5),
               "s16": (("peaked",), 6.0)}


@pytest.mark.parametrize("fault", list(RHO_REJECTS))
def test_rho_rejects(fault):
    regimes, least = RHO_REJECTS[fault]
    for key in _model_cases((XCD,)):
        case, r, rho = A.model_case(*key)
        got, worst = A.model_stats(A.emulate(case, key[4], fault=fault), r,
                                   key[3])
        if key[0] in regimes:
            assert got > least * rho > A.RHO_MARGIN * rho, (key, got / rho)
        if fault in ("scale16", "qscale16") and key[0] == "flat_offset":
            assert got < A.RHO_MARGIN * rho      # no shift on flat rows
        # the rigorous bound: o16 breaks it everywhere, s16 on peaked rows
        if fault == "o16" or (fault == "s16" and key[0] == "peaked"):
            assert worst > 1.5, (key, worst)


def test_slack_is_twice_the_measured_worst():
    """fp32 arithmetic in the kernel's order with P left unrounded, against
    fp64, in units of U * sum P |v|."""
    worst = 0.0
    for key in _model_cases():
        case, r, _ = A.model_case(*key)
        raw = A.emulate(case, key[4], raw=True, round_p=False)
        err = (raw.double() - r["ref"]).abs() / (A.U[key[3]] * r["pav"])
        worst = max(worst, err.max().item())
    assert 0.8 * A.SLACK_MEASURED <= worst <= A.SLACK_MEASURED, worst
    assert 2 * A.SLACK_MEASURED <= A.SLACK <= 2.1 * A.SLACK_MEASURED


def test_fp16_underflow_term_is_needed_and_small():
    """The 2^-25 sum |v_j| / l term: on flat rows it is at most 3% of the
    P-rounding term; on peaked rows it can be the larger of the two (the one
    heavy key has a V near 0, l is near 1, and 300 keys stand at 2^-25 each).
    It is what P below 2^-14 costs: with V = 1 and
    scores that put every P but one at 2^-15.5, the emulation's error is
    beyond the bound without the term and within it with the term."""
    for key in _model_cases((XCD,)):
        if key[3] == C.F16:
            _, r, _ = A.model_case(*key)
            part = (2.0 ** -25 * r["sav_l"] / (A.U[C.F16] * r["pav"])).max()
            if key[0] == "flat_offset":
                assert part < 0.05
    D = 64
    q = torch.zeros(1, 1, 4, D)
    k = torch.zeros(1, 1, A.SK, D)
    q[..., 0] = 8.0
    k[0, 0, 1:, 0] = -15.5 / A.LOG2E       # scaled score -15.5 log2 units
    case = dict(q=q.half(), k=k.half(), v=torch.ones(1, 1, A.SK, D).half(),
                keys=None, block=None)
    case["v"][0, 0, 0] = 0                 # the one large P carries nothing
    r = A.reference64(case)
    raw = A.emulate(case, raw=True)
    err = (raw.double() - r["ref"]).abs()
    assert (err > (1 + A.SLACK) * A.U[C.F16] * r["pav"]).all()
    assert (err <= (1 + A.SLACK) * A.U[C.F16] * r["pav"]
            + 2.0 ** -25 * r["sav_l"]).all()


# ------------------------------------------------- ops.attention* on the CPU

@DT
@DIMS
def test_ops_on_the_cpu_pass_the_exact_checks(D, dtype):
    """The reference path through every route of the GPU file."""
    for qmul in A.Q_SCALES:
        for mask in (None, "keys"):
            case = A.constant_columns(*XCD, D, dtype, qmul, mask=mask)
            for route in ("bhsd", "bshd", "split7", "split256"):
                A.check_constant(A.run_ops(case, route), case, route)
    case = A.constant_columns(0, 0, D, dtype, 3.0, mask="block")
    A.check_constant(A.run_ops(case), case, "block")
    case = A.constant_columns(*XCD, D, dtype, 3.0, Sq=A.FUSED_S, mask="keys")
    A.check_constant(A.run_ops(case, "fused"), case, "fused")
    Dp = C.PAD_DIMS[C.DIMS.index(D)]
    case = A.constant_columns(*A.GRIDS[1], Dp, dtype, 3.0, mask="keys")
    A.check_constant(A.run_ops(case, "bshd"), case, f"D={Dp}")
    for variant in A.GATHER_VARIANTS:
        for d in (D, Dp):
            case = A.one_hot_gather(variant, *XCD, d, dtype)
            seen = A.check_gather(A.run_ops(case, "bshd"), case, variant)
            assert seen["subnormal_flushed"] == 0


@GRID
def test_ops_on_the_cpu_pass_the_rounding_model(grid):
    for key in _model_cases((grid,)):
        case, r, rho = A.model_case(*key)
        got, worst = A.check_model(A.run_ops(case, scale=key[4]), r, key[3],
                                   A.RHO_MARGIN * rho, str(key))
        assert got <= rho * 1.001 and worst <= 0.51      # one rounding only


# ----------------------------------------------------- refusals and empties

def _qkv(B=2, H=3, Sq=5, Sk=9, D=8):
    g = C._gen(1)
    return (torch.randn(B, H, Sq, D, generator=g),
            torch.randn(B, H, Sk, D, generator=g),
            torch.randn(B, H, Sk, D, generator=g))


def _calls(q, k, v, **kw):
    qs, ks, vs = (t.permute(0, 2, 1, 3) if t.dim() == 4 else t
                  for t in (q, k, v))
    return (lambda: R.attention(q, k, v, **kw),
            lambda: ops.attention(q, k, v, **kw),
            lambda: ops.attention_bshd(qs, ks, vs, **kw),
            lambda: ops.attention_bshd_split(qs, ks, vs, 2, **kw))


MISMATCHES = {
    "k batch": (lambda q, k, v: (q, k[:1], v), "batch"),
    "v batch": (lambda q, k, v: (q, k, v[:1]), "batch"),
    "kv batch": (lambda q, k, v: (q, k[:1], v[:1]), "batch"),
    "k heads": (lambda q, k, v: (q, k[:, :1], v), "heads"),
    "kv heads": (lambda q, k, v: (q, k[:, :1], v[:, :1]), "heads"),
    "v heads": (lambda q, k, v: (q, k, v[:, :2]), "heads"),
    "k dim": (lambda q, k, v: (q, k[..., :4], v), "head dim"),
    "v dim": (lambda q, k, v: (q, k, v[..., :4]), "head dim"),
    "kv dim": (lambda q, k, v: (q, k[..., :4], v[..., :4]), "head dim"),
    "v length": (lambda q, k, v: (q, k, v[:, :, :8]), "length"),
    "3-D": (lambda q, k, v: (q, k[0], v[0]), "4-D"),
}


@pytest.mark.parametrize("name", list(MISMATCHES))
def test_mismatched_kv_is_refused_on_the_cpu(name):
    """k and v with q's batch, heads and head dim or a ValueError: the
    reference used to broadcast a batch-1 or head-1 k and v, which the
    native kernel reads past the end of. Masked calls refuse before any
    mask is packed."""
    make, word = MISMATCHES[name]
    q, k, v = make(*_qkv())
    masks = [dict(), dict(key_mask=torch.ones(2, 9, dtype=torch.bool))]
    for kw in masks:
        for call in _calls(q, k, v, **kw):
            with pytest.raises(ValueError, match=word):
                call()


@pytest.mark.parametrize("split", [0, 5, 6, -1])
def test_split_outside_the_rows_is_refused_on_the_cpu(split):
    qs, ks, vs = (t.permute(0, 2, 1, 3) for t in _qkv())
    with pytest.raises(ValueError, match="split"):
        ops.attention_bshd_split(qs, ks, vs, split)
    a, b = ops.attention_bshd_split(qs, ks, vs, 4)
    assert a.shape[1] == 4 and b.shape[1] == 1


@pytest.mark.parametrize("empty", ["B", "H", "Sq", "Sk"])
def test_empties_on_the_cpu(empty):
    """B, H or Sq of zero: the empty result. Sk = 0: zeros, the contract of
    a row that sees no key; with a key or block mask too."""
    dims = dict(B=2, H=3, Sq=5, Sk=9)
    dims[empty] = 0
    q, k, v = _qkv(**dims)
    want = torch.zeros_like(q)
    kms = [dict(), dict(key_mask=torch.ones(dims["B"], dims["Sk"],
                                            dtype=torch.bool))]
    for kw in kms:
        calls = _calls(q, k, v, **kw)
        for call in calls[:2]:
            assert torch.equal(call(), want)
        assert torch.equal(calls[2](), want.permute(0, 2, 1, 3))
        if empty == "Sq":
            with pytest.raises(ValueError, match="split"):
                calls[3]()
        else:
            a, b = calls[3]()
            assert torch.equal(torch.cat([a, b], 1),
                               want.permute(0, 2, 1, 3))
