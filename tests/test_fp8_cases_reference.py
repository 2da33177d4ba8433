"""The fp8 emit checks of fp8_cases.py discriminate (CPU, runs anywhere).

test_gpu_fp8_exact.py runs the native kernels through fp8_cases.CHECKS.
Here a plain-torch emulation of the kernels stands in for them, at the same
shapes and through the same checks: the faithful emulation passes every
check, every injected fault is rejected by the check named for it below,
and the conditions that make the checks sound are asserted on the
references alone (the grid encoder against torch's cast, the 5% cap on what
the off-tie criterion leaves out, the large pattern's rows).

With a builder replaced by plain randn (0.02 * randn in bf16, the same
length) this file fails 1 test for `ties` (the input conditions) and 2 for
`every_code` (the input conditions, and the faithful run, whose bytes are
no longer FINITE_BYTES). Every fault is still rejected: under byte equality
bf16 data at a power-of-two scale finds truncation on every second element
and sits on a tie on one element in sixteen (eight significant bits into
four). What the builders add is certainty, each code and each tie once,
where rel-l2 on the same randn could not see any of it.
"""
import pytest
import torch

import fp8_cases as F8
import kernel_cases as C

# fault -> the check that must reject it
REJECTED_BY = {
    "truncate": "quant ties scale=2^-7",
    "ties_away": "quant ties scale=2^-7",
    "subnormals_flushed": "quant every_code scale=2^-7",
    "no_clamp": "quant saturation_edge scale=2^-7",
    "clamp_240": "quant every_code scale=2^-7",
    "nan_to_min": "quant all_bf16 scale=0.012",
    "neg_zero_lost": "quant every_code scale=2^-7",
    "amax_overwritten": "quant prior first above",
    "amax_no_abs": "quant prior middle below",
    "snan_resets_amax": "quant all_bf16 scale=0.012",
    "no_decay": "quant sequence",
    "scale_undecayed": "quant sequence",
    "late_snapshot": "quant sequence",
    "no_floor": "quant floor",
    "last_vector_skipped": "quant every_code scale=2^-7",
    "ilp_slot_skipped": "large quant",
    "ilp_slots_swapped": "large quant",
    "inf_accepted": "quant nonfinite",
}
# rejected by the fused ops' checks too: the criterion that replaces byte
# equality there still sees them
ALSO_REJECTED_BY = {
    "truncate": "gelu all_finite_bf16 scale=0.012",
    "subnormals_flushed": "ln 2x5x3072 plain subnormal",
    "clamp_240": "gelu all_finite_bf16 scale=0.37",
    "nan_to_min": "ln nan_row",
    "amax_overwritten": "ln prior last above",
    "no_decay": "gelu all_finite_bf16 scale=2^-7",
    "late_snapshot": "ln 1x1x8 plain plain",
    "inf_accepted": "gelu nan_inf",
    "ilp_slots_swapped": "large gelu",
    "last_vector_skipped": "large gelu",
}


def _passes(name, fault=None):
    try:
        F8.CHECKS[name](F8.Emulated(fault))
    except AssertionError:
        return False
    return True


def test_fault_tables_cover_every_fault():
    assert set(REJECTED_BY) == set(F8.FAULTS) and len(F8.FAULTS) == 18
    assert set(REJECTED_BY.values()) | set(ALSO_REJECTED_BY.values()) <= set(
        F8.CHECKS)


@pytest.mark.parametrize("name", sorted(F8.CHECKS))
def test_faithful_emulation_passes(name):
    F8.CHECKS[name](F8.Emulated())


@pytest.mark.parametrize("fault", F8.FAULTS)
def test_fault_is_rejected(fault):
    assert not _passes(REJECTED_BY[fault], fault), \
        f"{fault} passes {REJECTED_BY[fault]}"


@pytest.mark.parametrize("fault", sorted(ALSO_REJECTED_BY))
def test_fault_is_rejected_by_a_fused_check(fault):
    assert not _passes(ALSO_REJECTED_BY[fault], fault), \
        f"{fault} passes {ALSO_REJECTED_BY[fault]}"


# ------------------------------------------------------ the references

def test_grid():
    g = F8.GRID
    assert g[0] == 0 and g[1] == 2.0 ** -9 and g[7] == 7 * 2.0 ** -9
    assert g[8] == 2.0 ** -6 and g[0x7E] == 448 and g[0x80] == 0
    assert torch.signbit(g[0x80]) and g[0x7F].isnan() and g[0xFF].isnan()
    assert len(F8.FINITE_BYTES) == 254
    assert (F8.POS[1:] > F8.POS[:-1]).all()
    assert torch.equal(g[128:255], -g[:127])
    # the spacing function is the distance to the next code
    assert torch.equal(F8.spacing(F8.POS[:-1]), F8.POS[1:] - F8.POS[:-1])
    assert F8.spacing(torch.tensor([2.0 ** -10, 17.0, 447.0])).tolist() == [
        2.0 ** -9, 2.0, 32.0]


def test_torch_cast_rounds_to_nearest_even():
    """The anchors emit_bytes rests on."""
    one = torch.ones(1)

    def byte(v):
        return int(F8.emit_bytes(torch.tensor([v]), one)[0])

    def value(v):
        return F8.GRID[byte(v)].item()

    assert value(17.0) == 16.0 and value(19.0) == 20.0
    assert byte(2.0 ** -10) == 0x00
    assert byte(float(torch.nextafter(torch.tensor(2.0 ** -10),
                                      torch.tensor(1.0)))) == 0x01
    assert byte(-0.0) == 0x80 and byte(-(2.0 ** -10)) == 0x80
    assert F8.is_nan_byte(torch.tensor(byte(float("nan"))))
    assert byte(float("inf")) == 0x7E and byte(-float("inf")) == 0xFE
    assert byte(464.0) == 0x7E and byte(1e30) == 0x7E


@pytest.mark.parametrize("scale", sorted(F8.SCALES))
def test_grid_encoder_is_torchs_cast(scale):
    """encode() walks the grid; on every bf16 pattern times every scale it
    gives torch's byte (NaN payloads aside)."""
    x = F8.all_bf16().float()
    s = F8.f32(F8.SCALES[scale])
    v = x * (torch.ones((), dtype=torch.float32) / s)
    F8.same_bytes(F8.encode(v), F8.emit_bytes(x, s), scale)


def test_every_code_and_tie_inputs():
    x = F8.every_code()
    assert x.numel() % 8 == 0
    assert torch.equal(F8.emit_bytes(x, F8.f32(F8.UNIT))[:254],
                       F8.FINITE_BYTES)
    assert x[-1] != 0                       # the last vector shows a skip
    t = F8.ties().double() / F8.UNIT
    assert t.numel() % 8 == 0
    n = len(F8.BOUNDARIES) - 1
    up = t[:3 * n].view(3, n)
    assert torch.equal(up[1], F8.BOUNDARIES[:-1]) and up[1, 0] == 2.0 ** -10
    assert (up[0] < up[1]).all() and (up[1] < up[2]).all()
    # the neighbours round to the two codes the tie lies between
    assert torch.equal(F8.GRID[F8.encode(up[0]).long()].double(), F8.POS[:-1])
    assert torch.equal(F8.GRID[F8.encode(up[2]).long()].double(), F8.POS[1:])
    # ties to even: the code with an even byte
    assert (F8.encode(up[1]) % 2 == 0).all()
    assert torch.equal(t[3 * n:6 * n], -t[:3 * n])
    e = F8.saturation_edge().float() / F8.UNIT
    assert e[:7].tolist()[:4] == [448.0, 448.0, 464.0, 464.0]
    assert e[6] == float("inf") and e[13] == -float("inf")
    assert F8.all_finite_bf16().numel() == 65280


def test_large_pattern_rows_differ_across_ilp_slots():
    pat = F8.large_pattern()
    want = F8.emit_bytes(pat, F8.f32(F8.UNIT))
    # rows pairwise different, bytes included
    assert torch.unique(want, dim=0).shape[0] == F8.PERIOD
    assert F8.LARGE_NVEC == 4096 * 256 * 5 + 5
    # the vectors of a thread lie GRID_VECS apart and 8191 is coprime to it
    steps = (torch.arange(1, 6) * F8.GRID_VECS) % F8.PERIOD
    assert (steps != 0).all() and torch.unique(steps).numel() == 5
    sat = ((want & 0x7F) == F8.MAX_BYTE).float().mean().item()
    assert 0.02 < sat < 0.3


@pytest.fixture(scope="module")
def offtie_cases():
    return list(F8.offtie_cases())


def test_offtie_exclusions_stay_under_the_cap(offtie_cases):
    for name, v64, _ in offtie_cases:
        share = F8.excluded_share(v64)
        assert share <= F8.EXCLUDED_CAP, f"{name}: {share:.4f} left out"
    assert len(offtie_cases) == 1 + 3 + len(F8.LN_CASES) + 2


def _error_in_spacings(v32, v64):
    e = (v32 - v64).abs() / F8.spacing(v64)
    return torch.where(v64.isfinite() & v32.isfinite(), e,
                       torch.zeros_like(e)).max().item()


def test_faithful_emulation_stays_a_quarter_of_the_margin(offtie_cases):
    """The criterion is sound for fp32 arithmetic on these cases with room
    to spare: the emulated kernels (single-pass LayerNorm statistics with
    either rounding of x * x + s, En * r GELU) are never more than a quarter
    of the margin from the fp64 value. Measured: 0.0006 spacings at most
    (ln 2x3x2056 plain plain); the margin is 0.0156."""
    for name, v64, v32 in offtie_cases:
        e = _error_in_spacings(v32, v64)
        assert e <= F8.MARGIN / 4, f"{name}: {e:.4f} spacings"
    for shape, rows, mod in F8.LN_CASES:
        x, sc, sh, q = F8.ln_case(shape, rows, mod)
        y64 = C.layer_norm_mod_f64(x, sc, sh, F8.LN_EPS)
        y32 = F8.ln_f32(x, sc, sh, fused=False)
        e = _error_in_spacings(F8.scaled64(y32.double(), F8.f32(q)),
                               F8.scaled64(y64, F8.f32(q)))
        assert e <= F8.MARGIN / 4, f"{shape} {rows} {mod}: {e:.4f} spacings"


def test_cancelling_gelu_tail_exceeds_the_margin():
    """Why gelu_fp8 takes En * r on the negative side: with 1 - r the fp32
    value is more than a whole margin from the fp64 one around x = -5."""
    x = F8.all_finite_bf16()
    v64 = F8.scaled64(F8.gelu_f64(x), F8.f32(F8.UNIT))
    old = F8.scaled64(F8.gelu_f32(x, cancelling=True).double(),
                      F8.f32(F8.UNIT))
    new = F8.scaled64(F8.gelu_f32(x).double(), F8.f32(F8.UNIT))
    assert _error_in_spacings(old, v64) > F8.MARGIN
    assert _error_in_spacings(new, v64) < F8.MARGIN / 16


def test_offtie_mask():
    v = torch.tensor([16.0, 17.0, 17.0 + 2.0 / 64 * 1.01, 17.0 + 2.0 / 64 * 0.99,
                      464.0, 463.9, 2.0 ** -10, 0.0, float("nan"),
                      float("inf"), 1e4], dtype=torch.float64)
    assert F8.offtie_mask(v).tolist() == [
        True, False, True, False, False, False, False, True, False, True,
        True]
    assert torch.equal(F8.offtie_mask(-v), F8.offtie_mask(v))


def test_delayed_scale_recurrence():
    st = F8.DelayedScale(0.5, amax=2.0)
    st.update(F8.f32(3.0))
    a = F8.f32(3.0) * F8.f32(0.999)
    assert st.used[0] == 0.5 and st.amax[0] == a and st.amax[1] == 0
    assert st.scale[0] == a / F8.f32(448.0)
    st.update(F8.f32(1.0))                          # below the running amax
    assert st.amax[0] == a * F8.f32(0.999)
    st.update(F8.f32(float("inf")))                 # the non-finite rule
    s = a * F8.f32(0.999) / F8.f32(448.0)
    assert st.scale[0] == s and st.amax[0] == s * F8.f32(448.0)
    one = F8.DelayedScale(0.5, amax=2.0, slots=1).update(F8.f32(3.0))
    assert one.amax.tolist() == [3.0] and one.scale[0] == 0.5
