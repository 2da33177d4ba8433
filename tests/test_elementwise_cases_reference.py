"""The checks of elementwise_cases.py discriminate (CPU, runs anywhere).

test_gpu_elementwise_exact.py runs the native kernels through
elementwise_cases.CHECKS. Here a plain-torch emulation of the kernels' index
arithmetic and fp32 evaluation order stands in for them, at the same shapes
and through the same checks: the faithful emulation passes every check,
every injected fault is rejected by the check named for it below, and ops.*
on the CPU passes them too, refusals and empties included, so the reference
path keeps the contract the kernels are held to. The constants of the two
criteria (SLACK, TS_A, TS_B) are measured here against their recorded
values.

With one builder replaced by the inputs of the earlier tests (randn rows, a
rope_freqs(arange(S)) table, t = rand) the file fails; WITH_OLD lists, per
builder, which tests, and the faults that then pass the check named for
them (test_old_builder_is_caught).
"""
import pytest
import torch

import elementwise_cases as E
from comfyui_parallelanything_amd import ops

# (family, fault) -> the check that must reject it
REJECTED_BY = {
    ("qk", "cs_row_next"): "qk fused quarter D=128 bf16",
    ("qk", "cs_row_prev"): "qk permuted quarter D=64 fp16",
    ("qk", "cs_by_row"): "qk sliced quarter D=40 bf16",
    ("qk", "pair_shifted"): "qk fused quarter D=40 fp16",
    ("qk", "upper_unrotated"): "qk permuted quarter D=128 bf16",
    ("qk", "direction_flipped"): "qk sliced quarter D=2 bf16",
    ("qk", "w0_w1_swapped"): "qk permuted model D=128 bf16",
    ("qk", "wq_for_k"): "qk sliced model D=40 bf16",
    ("qk", "batch_stride_ignored"): "qk permuted quarter D=64 bf16",
    ("qk", "tail_rows_stored"): "qk fused quarter D=128 fp16",
    ("qk", "dead_lanes_stored"): "qk sliced quarter D=40 bf16",
    ("pack", "img_cs_local"): "pack 3x2x3x3 img_sliced quarter D=128 bf16",
    ("pack", "boundary_late"): "pack 3x2x3x3 txt_sliced quarter D=40 bf16",
    ("pack", "boundary_early"): "pack 3x2x3x3 img_sliced quarter D=40 fp16",
    ("pack", "txt_weights_on_img"):
        "pack 3x2x3x3 img_sliced quarter D=128 fp16",
    ("pack", "qkv_stride_swapped"): "pack 3x2x3x3 txt_sliced model D=40 bf16",
    ("pack", "local_order"): "pack 3x2x3x3 txt_sliced quarter D=128 bf16",
    ("rope", "s_without_mod"): "rope quarter D=6 bf16",
    ("rope", "h_ignored"): "rope quarter D=64 fp16",
    ("rope", "last_trip_skipped"): "rope large bf16",
    ("rope", "second_trip_reads_first"): "rope large fp32",
    ("gate", "b_from_wrong_S"): "gate vec bf16",
    ("gate", "d_wrong_modulus"): "gate large_scalar bf16",
    ("gate", "gate_row_0"): "gate scalar fp32 unbind",
    ("gate", "last_vector_skipped"): "gate vec fp16 unbind",
    ("gate", "last_trip_skipped"): "gate large_vec bf16",
    ("ts", "no_range_reduction"): "ts dim=256 P=10000",
    ("ts", "argument_clamped"): "ts dim=320 P=100",
    ("ts", "halves_swapped"): "ts dim=2 P=10000",
    ("ts", "half_from_dim"): "ts dim=256 P=100",
    ("ts", "odd_column_unwritten"): "ts dim=3 P=10000",
    ("mlp", "b_from_block"): "mlp K=256",
    ("mlp", "halves_swapped"): "mlp K=8",
    ("mlp", "tail_block_past_H"): "mlp K=256 bias",
    ("mlp", "lds_fill_stops_at_256"): "mlp K=1024",
}
# a second check each for the faults the issue singles out
ALSO_REJECTED_BY = {
    ("ts", "no_range_reduction"): "mlp K=256",
    ("ts", "argument_clamped"): "ts large",
    ("qk", "upper_unrotated"): "qk fused quarter D=40 bf16",
    ("qk", "tail_rows_stored"): "qk sliced model D=64 bf16",
    ("gate", "last_trip_skipped"): "gate large_scalar fp32",
    ("gate", "d_wrong_modulus"): "gate vec bf16 unbind",
}
ALL_FAULTS = [(fam, f) for fam, fs in E.FAULTS.items() for f in fs]


def _id(fault):
    return "-".join(fault)


def _passes(name, fault=None, **kw):
    if fault is not None and fault[0] == "ts" and name.startswith("mlp"):
        # the fused kernel holds the same sinusoid
        be = E.Emulated(fault)
        be.timestep_embed_mlp = lambda t, w1, b1, P, tf: _mlp_with_ts_fault(
            t, w1, b1, P, tf, fault[1])
    else:
        be = E.Emulated(fault, **kw)
    try:
        E.CHECKS[name](be)
    except AssertionError:
        return False
    return True


def _mlp_with_ts_fault(t, w1, b1, P, tf, fault):
    emb = E.emulate_timestep_embedding(t, w1.shape[1], P, tf, fault)
    acc = emb @ w1.float().t() + (0 if b1 is None else b1.float())
    return torch.nn.functional.silu(acc).to(E.BF16)


def test_fault_tables_cover_every_fault():
    assert set(REJECTED_BY) == set(ALL_FAULTS) and len(ALL_FAULTS) == 35
    assert set(REJECTED_BY.values()) | set(ALSO_REJECTED_BY.values()) <= set(
        E.CHECKS)
    assert len(E.CHECKS) == 153


@pytest.mark.parametrize("name", sorted(E.CHECKS))
def test_faithful_emulation_passes(name):
    E.CHECKS[name](E.Emulated())


@pytest.mark.parametrize("name", sorted(
    n for n in E.CHECKS if n.startswith(("qk", "pack", "rope model"))))
def test_unfused_and_off_by_an_ulp_emulations_pass(name):
    """The criterion may not hang on what the emulation cannot know: mul +
    add in place of fma, the reciprocal square root an fp32 ulp off."""
    E.CHECKS[name](E.Emulated(fused=False, rsq_ulp=1))
    E.CHECKS[name](E.Emulated(fused=True, rsq_ulp=-1))


@pytest.mark.parametrize("fault", ALL_FAULTS, ids=_id)
def test_fault_is_rejected(fault):
    assert not _passes(REJECTED_BY[fault], fault), \
        f"{fault} passes {REJECTED_BY[fault]}"


@pytest.mark.parametrize("fault", sorted(ALSO_REJECTED_BY), ids=_id)
def test_fault_is_rejected_by_a_second_check(fault):
    assert not _passes(ALSO_REJECTED_BY[fault], fault), \
        f"{fault} passes {ALSO_REJECTED_BY[fault]}"


# ------------------------------------------------- the two criteria

def test_slack_is_twice_the_measured_worst():
    """The faithful emulation, with either multiply-add and the reciprocal
    square root an ulp either way, stays within half the chosen SLACK of
    fp64 before the final rounding, and SLACK_MEASURED is what is measured
    here."""
    rows = list(E.slack_measurements())
    assert len(rows) == 2 * (4 * 7 + 2 + 3)
    name, worst = max(rows, key=lambda r: r[1])
    assert worst <= E.SLACK / 2, f"{name}: {worst:.4f} spacings"
    assert abs(worst - E.SLACK_MEASURED) <= 1e-4, f"{name}: {worst:.5f}"
    assert 2 * E.SLACK_MEASURED <= E.SLACK <= 2.1 * E.SLACK_MEASURED


def test_ts_bound_is_four_times_the_measured_one():
    a, b = E.ts_measurements()
    assert a <= E.TS_A_MEASURED * 1.001 and b <= E.TS_B_MEASURED * 1.001, (
        a, b)
    assert a >= E.TS_A_MEASURED * 0.99 and b >= E.TS_B_MEASURED * 0.99, (a, b)
    assert 4 * E.TS_A_MEASURED <= E.TS_A <= 4.05 * E.TS_A_MEASURED
    assert 4 * E.TS_B_MEASURED <= E.TS_B <= 4.05 * E.TS_B_MEASURED


def test_spacing16():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 0.0, 2.0 ** -20, 65504.0],
                     dtype=torch.float64)
    assert E.spacing16(v, E.BF16).tolist() == [
        2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 2.0 ** -133,
        2.0 ** -27, 2.0 ** 8]
    assert E.spacing16(v, E.F16).tolist() == [
        2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -9, 2.0 ** -24,
        2.0 ** -24, 2.0 ** 5]
    # it is the distance to the next value of the type
    for dtype in (E.BF16, E.F16):
        x = torch.tensor([1.0, 0.3, 100.0]).to(dtype)
        nxt = (x.view(torch.int16) + 1).view(dtype)
        assert torch.equal(E.spacing16(x.double(), dtype),
                           nxt.double() - x.double())


# ------------------------------------------------- the inputs

def _quarter_turns():
    cs = E.build("quarter_table", 19, 64)
    assert torch.equal(cs[..., 0] ** 2 + cs[..., 1] ** 2, torch.ones(19, 64))
    kinds = (cs[..., 0] + 2 * cs[..., 1]).long()       # 1, 2, -1, -2
    for s in range(19):                 # every turn in both halves of a row
        assert set(kinds[s, :32].tolist()) == {1, 2, -1, -2}
        assert set(kinds[s, 32:].tolist()) == {1, 2, -1, -2}
    assert torch.unique(kinds, dim=0).shape[0] == 19
    # the old table leaves the upper pairs almost unturned: the gap
    old = E.OLD_BUILDERS["quarter_table"](5, 64)
    assert old[:, 43:, 1].abs().max() < 0.01           # the upper third


def _unit_rows():
    for D in E.QK_DIMS:
        x = E.build("unit_rows", (3, 5, 3, D), E.BF16, 1).float()
        assert torch.equal((x * x).sum(-1), torch.full((3, 5, 3), float(D)))
        if D >= 40:
            assert torch.unique(x.view(-1, D), dim=0).shape[0] == 45


def _pow2_rows():
    x = E.build("pow2_rows", (3, 5, 24), E.F16, 50).double()
    m, e = torch.frexp(x.abs())
    assert (m == 0.5).all() and e.min() == 0 and e.max() == 2
    assert (x < 0).any() and (x > 0).any()


def _spread():
    x = E.build("spread", (45, 128), E.BF16, 1).double().abs()
    assert x.min() >= 2.0 ** -3 and x.max() <= 2.0 ** 3
    assert x.log2().std() > 1.5         # not one scale: 1.73 for 6 octaves


def _model_table():
    """Three axes: text rows turn on axis 0 alone, image rows on the
    others, and the slice the models pass starts at the first image row."""
    cs = E.build("model_table", 128)
    assert cs.shape == (19, 64, 2) and cs.dtype == torch.float32
    assert (cs[:7, 8:, 0] == 1).all() and (cs[:7, 8:, 1] == 0).all()
    assert (cs[7:, :8, 0] == 1).all() and (cs[1:7, :8, 1] != 0).all()
    assert torch.equal(E.build("model_table", 128, 7), cs[7:])
    assert (cs[7 + 4:, 8:36, 1] != 0).all()      # rows 1, 2 of the grid


def _wan_table():
    cs = E.build("wan_table", 128)               # 2 frames of 2 x 3
    assert cs.shape == (12, 64, 2)
    assert (cs[:6, :8, 0] == 1).all() and (cs[6:, :8, 1] != 0).all()
    assert torch.equal(cs[0, 36:], cs[3, 36:])   # the column axis repeats
    assert not torch.equal(cs[0, 36:], cs[1, 36:])


def _ts_arguments():
    for t, tf in E.build("ts_arguments"):
        a = (t.double() * tf).abs()
        assert (a > E.REV256).sum() == 4 and (a < E.REV256).sum() == 6
        assert abs(a.max() - 14610.0) < 1e-2 and (t < 0).any()
        assert ((a > 1590) & (a < E.REV256)).any()
        assert ((a > E.REV256) & (a < 1620)).any()


INPUT_CONDITIONS = {"quarter_table": _quarter_turns, "unit_rows": _unit_rows,
                    "pow2_rows": _pow2_rows, "spread": _spread,
                    "model_table": _model_table, "wan_table": _wan_table,
                    "ts_arguments": _ts_arguments}


@pytest.mark.parametrize("builder", sorted(INPUT_CONDITIONS))
def test_input_conditions(builder):
    INPUT_CONDITIONS[builder]()


def test_guards_and_v_patterns():
    for dtype in (E.BF16, E.F16):
        g = E._guarded((4, 4), dtype)
        assert g.isnan().all()
        v = E._distinct((3, 5, 3, 128), dtype)      # 5760 patterns
        assert torch.unique(v.view(torch.int16)).numel() == v.numel()
        txt, img, ws, cs, eps, exact, v = E.pack_case(
            E.PACK_ALL16, "img_sliced", "quarter", 128, dtype)
        # every 16-bit pattern once: NaN payloads, -0 and infinities too
        assert torch.equal(v.view(torch.int16).flatten().sort().values,
                           torch.arange(-32768, 32768, dtype=torch.int16))
    # four distinct weights
    assert len({tuple(w.tolist()) for w in ws}) == 4


def test_large_shapes_take_a_second_trip():
    n = torch.tensor(E.ROPE_LARGE).prod().item() // 2
    assert n == 1049984 and E.GRID < n < 2 * E.GRID
    B, S, D = E.GATE_SHAPES["large_vec"]
    assert B * S * D == 8390656 and E.GRID < B * S * D // 8 < 2 * E.GRID
    B, S, D = E.GATE_SHAPES["large_scalar"]
    assert B * S * D == 1048660 and D % 8 != 0
    assert E.GRID < E.GELU_LARGE_VECS < 2 * E.GRID
    B, dim = E.TS_LARGE
    assert B * (dim // 2) > 1024 * 256
    assert E.PERIOD % 2 == 1            # coprime to the 2^20 items of a trip


# ------------------------------------------------- ops.* on the CPU

@pytest.fixture(scope="module")
def cpu_ops():
    return E.OpsBackend("cpu")


@pytest.mark.parametrize("name", sorted(E.CHECKS))
def test_cpu_ops_pass(name, cpu_ops):
    E.CHECKS[name](cpu_ops)


@pytest.mark.parametrize("name", sorted(E.REFUSALS))
def test_cpu_ops_refuse(name, cpu_ops):
    with pytest.raises(RuntimeError):
        E.REFUSALS[name](ops, "cpu")
    E.CHECKS[E.after_refusal(name)](cpu_ops)


@pytest.mark.parametrize("name", sorted(E.EMPTIES))
def test_cpu_ops_empties(name):
    E.EMPTIES[name](ops, "cpu")


def test_cpu_timestep_embedding_dim_1_is_the_zero_column():
    out = ops.timestep_embedding(torch.tensor([0.5, 4.0]), 1)
    assert out.shape == (2, 1) and (out == 0).all()


# ------------------------------------------------- the old inputs

# What fails, per builder, once it alone gives the inputs of the earlier
# tests (randn rows, a rope_freqs(arange(S)) table, t = rand(10)):
#   conditions  whether test_input_conditions[builder] fails
#   faithful    how many checks the faithful emulation then misses (the
#               exact cases are exact no longer), the large ones aside
#   slips       the faults that then pass the check named for them
#   slack       whether test_slack_is_twice_the_measured_worst fails
# The old tables and rows still show most index faults here, because the
# comparison is in spacings of the output and no longer atol = 2e-2; what
# they lose is exactness, the turned upper pairs, and everything beyond 256
# revolutions.
WITH_OLD = {
    "spread": dict(conditions=True, faithful=0, slips=[], slack=True),
    "unit_rows": dict(conditions=True, faithful=5, slips=[], slack=False),
    "pow2_rows": dict(conditions=True, faithful=4, slips=[], slack=False),
    "quarter_table": dict(conditions=True, faithful=0, slips=[],
                          slack=False),
    "model_table": dict(conditions=True, faithful=1, slips=[], slack=True),
    "wan_table": dict(conditions=True, faithful=0, slips=[], slack=False),
    "ts_arguments": dict(conditions=True, faithful=0,
                         slips=["ts-no_range_reduction",
                                "ts-argument_clamped"], slack=False),
}


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# the check families that draw on each builder, and whether the slack
# measurement does
USED_BY = {"spread": (("qk", "pack", "rope"), True),
           "unit_rows": (("qk", "pack"), False),
           "pow2_rows": (("rope", "gate"), False),
           "quarter_table": (("qk", "pack", "rope"), True),
           "model_table": (("qk", "pack", "rope"), True),
           "wan_table": (("qk",), True),
           "ts_arguments": (("ts", "mlp"), False)}


def survey_old_builder(builder, monkeypatch):
    monkeypatch.setitem(E.BUILDERS, builder, E.OLD_BUILDERS[builder])
    families, in_slack = USED_BY[builder]
    names = [n for n in sorted(E.CHECKS)
             if n not in E.LARGE and n.startswith(families)]
    faithful = [n for n in names if not _passes(n)]
    slips = [_id(f) for f in ALL_FAULTS
             if REJECTED_BY[f] in names and REJECTED_BY[f] not in faithful
             and _passes(REJECTED_BY[f], f)]
    return dict(conditions=_fails(INPUT_CONDITIONS[builder]),
                faithful=len(faithful), slips=slips,
                slack=in_slack
                and _fails(test_slack_is_twice_the_measured_worst))


@pytest.mark.parametrize("builder", sorted(E.BUILDERS))
def test_old_builder_is_caught(builder, monkeypatch):
    """With this builder alone giving the old inputs, tests of this file
    fail: WITH_OLD says which."""
    got = survey_old_builder(builder, monkeypatch)
    assert got["conditions"] or got["faithful"] or got["slips"]
    assert got == WITH_OLD[builder]
