"""CPU proof that tests/block_cases.py bites: the two fp64 references agree
at every tap of every block (and would not if any op rounded to fp32), the
16-bit reference path is a usable yardstick, and every injected wiring
fault moves a named tap by at least twice the limit the GPU run is held to
(tests/test_gpu_blocks.py). docs/KERNELS.md, "Block composition".
"""
import math

import pytest
import torch

import block_cases as C
from comfyui_parallelanything_amd import ops

CASE_IDS = [c.id for c in C.CASES]
DT_IDS = ["bf16", "fp16"]


def test_cases_cover_the_issue_geometry():
    """Two query blocks, a partial last tile, the txt/img boundary inside
    tile 0; frame edges inside KV tiles; the D = 40 pad route."""
    S = C.T_TXT + C.IMG_HW[0] * C.IMG_HW[1]
    assert S == 309 and ops.reference.block_mask_shape(S, S) == (2, 5)
    assert 0 < C.T_TXT < 64 and S % 64
    f, h, w = C.WAN_GRID
    assert f * h * w == 336 and (h * w) % 64
    assert {c.width // c.heads for c in C.cases("double", "single", "wan")} \
        == {64, 128}
    assert {c.width // c.heads for c in C.cases("sdtx")} == {40, 64}
    assert len(CASE_IDS) == len(set(CASE_IDS))


def test_recorder_restores_ops_and_names_taps():
    before = {n: getattr(ops, n) for n in C.RECORDED}
    taps = C.reference(C.build(C.cases("double")[0], C.BF16))
    assert {n: getattr(ops, n) for n in C.RECORDED} == before
    assert list(taps) == [
        "layer_norm_mod#0[0]", "layer_norm_mod#1[0]",
        "pack_joint_qkv#0[0]", "pack_joint_qkv#0[1]", "pack_joint_qkv#0[2]",
        "attention_bshd_split#0[0]", "attention_bshd_split#0[1]",
        "gate_residual#0[0]", "layer_norm_mod#2[0]", "gate_residual#1[0]",
        "gate_residual#2[0]", "layer_norm_mod#3[0]", "gate_residual#3[0]",
        "out[0]", "out[1]"]
    assert all(t.dtype == torch.float64 for t in taps.values())


@pytest.mark.parametrize("dtype", C.DTYPES16, ids=DT_IDS)
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_fp64_references_agree(case, dtype):
    """The module in fp64 on the reference path against the composition
    written out with torch arithmetic: under 1e-9 at every tap, so the
    suite does not rest on ops.reference being right about itself."""
    built = C.build(case, dtype)
    err = C.errors(C.reference(built), C.compose(built))
    worst = max(err, key=err.get)
    assert err[worst] < C.FP64_AGREE, (case.id, worst, err[worst])


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_fp32_on_the_reference_path_would_show(case, monkeypatch):
    """With ops.reference._wide forced back to fp32 (what the reference path
    did before it kept fp64), the first tap an op produces lies about 7e-8
    from the fp64 run, not 1e-16: the 1e-9 of test_fp64_references_agree
    catches any op of any case that rounds to fp32, group_norm_silu and the
    attention of the SD blocks included."""
    built = C.build(case, C.BF16)
    ref = C.reference(built)
    monkeypatch.setattr(ops.reference, "_wide", lambda x: x.float())
    narrow = C.run(built, "cpu", C.F64)
    first = next(iter(narrow))
    assert not first.startswith("out"), first
    d = C.rel_l2(narrow[first], ref[first])
    assert 10 * C.FP64_AGREE < d < 1e-5, (case.id, first, d)
    assert C.rel_l2(narrow["out[0]"], ref["out[0]"]) > 10 * C.FP64_AGREE


@pytest.mark.parametrize("dtype", C.DTYPES16, ids=DT_IDS)
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_faults_exceed_twice_the_limit(case, dtype):
    """Every fault of the case, run in fp64, lies at least FAULT_FACTOR * M
    * e_ref(tap) from the clean fp64 run at one of the taps it names."""
    built = C.build(case, dtype)
    e_ref = C.e_ref(built)
    assert all(0 < e < 0.01 for e in e_ref.values()), e_ref
    margins = {}
    for fault in C.faults_for(case):
        d = C.fault_distance(built, fault)
        # every named tap was recorded; inf only where its shape changed
        assert set(fault.taps) <= set(d), (fault.name, fault.taps, list(d))
        assert fault.refused or all(math.isfinite(d[t]) for t in fault.taps)
        margins[fault.name] = max(d[t] / e_ref[t] for t in fault.taps)
    print(f"\nfault / e_ref {case.id} {DT_IDS[C.DTYPES16.index(dtype)]}: "
          + ", ".join(f"{n} {m:.2f}" for n, m in margins.items()))
    need = C.FAULT_FACTOR * C.M[dtype]
    weak = {n: round(m, 3) for n, m in margins.items() if not m >= need}
    assert not weak, f"{case.id}: faults under {need} x e_ref: {weak}"


def test_every_fault_is_used_and_every_kind_has_one():
    used = {f.name + "/" + k for c in C.CASES
            for f in C.FAULTS if f.applies(c) for k in (c.kind,)}
    assert used == {f.name + "/" + k for f in C.FAULTS for k in f.kinds}
    assert {k for f in C.FAULTS for k in f.kinds} == {
        "double", "single", "wan", "sdtx", "last"}


@pytest.mark.parametrize("case", C.cases(*C.MLP_KINDS), ids=lambda c: c.id)
def test_erf_gelu_exceeds_twice_the_fp32_limit(case):
    """erf-GELU for tanh-GELU is 1.8e-4 of the MLP branch, below 16-bit
    rounding; the fp32 limit M32 * e32_ref (the CPU fp32 run's distance
    from fp64) holds it, and with it the GPU-only _addmm_activation
    epilogue that the fp32 GPU run compares."""
    built = C.build(case, C.BF16)
    e32 = C.e_ref(built, C.F32)
    assert all(e < 5e-7 for e in e32.values()), e32
    faults = C.faults_for(case, fp32_only=True)
    assert faults
    for fault in faults:
        d = C.fault_distance(built, fault)
        for tap in fault.taps:
            assert d[tap] >= C.FAULT_FACTOR * C.M32 * e32[tap], (
                case.id, fault.name, tap, d[tap], e32[tap])


@pytest.mark.parametrize("dtype", C.DTYPES16, ids=DT_IDS)
@pytest.mark.parametrize("name", list(C.MODEL_CASES))
def test_whole_model_yardstick(name, dtype):
    """The CPU 16-bit forward of every whole-model case sits within a few
    roundings of fp64: the e_ref that M_MODEL multiplies."""
    ref = C.model_reference(name, dtype)
    assert ref.dtype == torch.float64 and torch.isfinite(ref).all()
    e = C.model_e_ref(name, dtype)
    eps = 2.0 ** -8 if dtype == C.BF16 else 2.0 ** -11
    assert 0.2 * eps < e < 4 * eps, (name, e)
