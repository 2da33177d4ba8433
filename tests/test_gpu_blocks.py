"""The model blocks on the native gfx950 path, stage by stage against fp64.

Cases, taps, references and the limits M / M32 / M_MODEL: tests/
block_cases.py; tests/test_block_cases_reference.py shows on the CPU that
every wiring fault listed there exceeds twice these limits. Run with -s for
the per-tap e_gpu / e_ref ratios. docs/KERNELS.md, "Block composition".
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import block_cases as C
from comfyui_parallelanything_amd import ops

DT_IDS = {C.BF16: "bf16", C.F16: "fp16"}
DTYPES = pytest.mark.parametrize("dtype", C.DTYPES16,
                                 ids=list(DT_IDS.values()))
# the extension entry points behind every recorded op (block_cases.RECORDED)
ENTRY_POINTS = ("attn_fwd_bshd", "attn_fwd_bshd_masked",
                "attn_fwd_bshd_split", "attn_fwd_bshd_split_masked",
                "pack_joint_qkv", "qk_norm_rope_", "layer_norm_mod",
                "gate_residual", "group_norm_silu", "rms_norm", "gelu_tanh")


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert all(ops.hip_available(n) for n in ENTRY_POINTS), (
        "native _pa_hip extension must be present")


@pytest.fixture()
def no_fallback(monkeypatch):
    """Fails the test if any op reported the reference path. gate_residual,
    rms_norm and gelu_tanh have no report to give: entry_counts holds every
    recorded op to the number of native launches the case must make."""
    seen = []
    orig = ops._unsupported

    def spy(op, why):
        seen.append((op, why))
        return orig(op, why)

    monkeypatch.setattr(ops, "_unsupported", spy)
    yield seen
    assert not seen, f"ops fell back to the reference path: {seen}"


@pytest.fixture()
def entry_counts(monkeypatch):
    """Calls per extension entry point of the recorded ops; the masked
    attention entry points count under '<name>/key' (2-D live lists) or
    '<name>/block' (3-D). No block calls rms_norm or gelu_tanh outside the
    fp8 mode, so either name in the counts fails the comparison."""
    ext = ops.hip_ext()
    counts = {}

    def wrap(name, fn):
        def counted(*args):
            key = name
            if name.endswith("_masked"):
                key += "/block" if args[-2].dim() == 3 else "/key"
            counts[key] = counts.get(key, 0) + 1
            return fn(*args)
        return counted

    for name in ENTRY_POINTS:
        monkeypatch.setattr(ext, name, wrap(name, getattr(ext, name)))
    return counts


def expected_entries(case):
    if case.kind == "double":
        return {("attn_fwd_bshd_split_masked/key" if case.masked
                 else "attn_fwd_bshd_split"): 1, "pack_joint_qkv": 1,
                "layer_norm_mod": 4, "gate_residual": 4}
    if case.kind == "single":
        return {("attn_fwd_bshd_masked/key" if case.masked
                 else "attn_fwd_bshd"): 1, "qk_norm_rope_": 1,
                "layer_norm_mod": 1, "gate_residual": 1}
    if case.kind == "wan":
        return {("attn_fwd_bshd_masked/block" if case.window is not None
                 else "attn_fwd_bshd"): 1,
                "attn_fwd_bshd_masked/key": 1, "qk_norm_rope_": 1,
                "layer_norm_mod": 2, "gate_residual": 2}
    if case.kind == "sdtx":
        return {"attn_fwd_bshd": 1, "attn_fwd_bshd_masked/key": 1}
    if case.kind == "last":
        return {"layer_norm_mod": 1}
    if case.kind == "res":
        return {"group_norm_silu": 2}
    raise ValueError(case.kind)


def _report(tag, e_gpu, e_ref):
    print(f"\n{tag}: " + ", ".join(
        f"{t} {e_gpu[t]:.3e}/{e_ref[t]:.3e}={e_gpu[t] / e_ref[t]:.3f}"
        for t in e_gpu))


# ---------------- a. stage limits ----------------

@DTYPES
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_stage_limits(case, dtype, no_fallback, entry_counts):
    """e_gpu(tap) <= M * e_ref(tap) at every tap, e_ref from the CPU run of
    the same 16-bit type, both measured from the fp64 run."""
    built = C.build(case, dtype)
    ref, e_ref = C.reference(built), C.e_ref(built)
    e_gpu = C.errors(C.run(built, "cuda", dtype), ref)
    _report(f"{case.id} {DT_IDS[dtype]}", e_gpu, e_ref)
    assert entry_counts == expected_entries(case), (case.id, entry_counts)
    for tap, e in e_gpu.items():
        assert e <= C.M[dtype] * e_ref[tap], (
            f"{case.kind} block, case {case.id} {DT_IDS[dtype]}: tap {tap} "
            f"is {e:.3e} from fp64, limit {C.M[dtype]} x {e_ref[tap]:.3e} "
            f"(ratio {e / e_ref[tap]:.3f})")


# ---------------- b. exact properties ----------------

_PAD_KEY = {"double": "txt", "single": "x", "wan": "context",
            "sdtx": "context"}
PAD_CASES = [c for c in C.CASES if c.masked and not c.banked
             and c.window is None and c.kind in _PAD_KEY]


def _fill_padded(kind, fill):
    """kw_edit: overwrite the padded text / context rows."""
    def edit(kw):
        t = kw[_PAD_KEY[kind]].clone()
        dead = ~C.text_mask(t.device)               # [B, T]
        rows = t[:, :C.T_TXT]
        if fill == "nan":
            rows[dead] = float("nan")
        else:
            g = torch.Generator(device="cpu").manual_seed(77)
            noise = 30.0 * torch.randn(int(dead.sum()), t.shape[-1],
                                       generator=g)
            rows[dead] = noise.to(t.device, t.dtype)
        return {**kw, _PAD_KEY[kind]: t}
    return edit


@DTYPES
@pytest.mark.parametrize("case", PAD_CASES, ids=lambda c: c.id)
def test_padded_rows_are_dont_care_end_to_end(case, dtype, no_fallback):
    """Padded context rows holding finite noise x 30 or NaN: every row that
    is not itself padding comes out bit-identical."""
    built = C.build(case, dtype)
    a = C.run(built, "cuda", dtype, kw_edit=_fill_padded(case.kind, "noise"))
    b = C.run(built, "cuda", dtype, kw_edit=_fill_padded(case.kind, "nan"))
    live = C.text_mask("cuda")
    if case.kind == "double":
        assert torch.equal(a["out[0]"], b["out[0]"])            # image
        assert torch.equal(a["out[1]"][live], b["out[1]"][live])
        assert b["out[1]"][~live].isnan().any()     # the NaN was there
    elif case.kind == "single":
        T = C.T_TXT
        assert torch.equal(a["out[0]"][:, T:], b["out[0]"][:, T:])
        assert torch.equal(a["out[0]"][:, :T][live], b["out[0]"][:, :T][live])
        assert b["out[0]"][:, :T][~live].isnan().any()
    else:
        assert torch.equal(a["out[0]"], b["out[0]"])
    assert torch.isfinite(a["out[0]"]).all()


@DTYPES
@pytest.mark.parametrize("kind,width,axes", [
    ("double", 256, (16, 56, 56)), ("double", 128, (16, 24, 24)),
    ("single", 256, (16, 56, 56)), ("single", 128, (16, 24, 24))])
def test_all_true_mask_equals_no_mask(kind, width, axes, dtype, no_fallback,
                                      entry_counts):
    """S = 48 + 272 = 320, a multiple of 64: the masked kernel walks the
    unmasked kernel's tile sequence, so an all-true attention_mask changes
    no bit of the block's output."""
    from comfyui_parallelanything_amd.models.layers import joint_key_mask
    case = C.Case(kind, width, 2, axes, txt=48)
    built = C.build(case, dtype)

    def all_true(kw):
        am = torch.ones(C.BATCH, 48, dtype=torch.bool, device="cuda")
        return {**kw, "key_mask": joint_key_mask(
            am, C.BATCH, 48, C.IMG_HW[0] * C.IMG_HW[1])}

    plain = C.run(built, "cuda", dtype)
    masked = C.run(built, "cuda", dtype, kw_edit=all_true)
    attn = "attn_fwd_bshd_split" if kind == "double" else "attn_fwd_bshd"
    assert entry_counts[attn] == 1 and entry_counts[attn + "_masked/key"] == 1
    for tap in plain:
        assert torch.equal(plain[tap], masked[tap]), tap


@DTYPES
def test_frame_window_over_every_frame_is_dense(dtype, no_fallback,
                                                entry_counts):
    """WanDiT._frame_window_mask: a window that reaches every frame (>=
    frames - 1) packs no mask, and the forward is the dense one bit for
    bit; window 1 packs one and differs."""
    def window(w):
        def prepare(model):
            model.cfg.self_attn_frame_window = w
            prepare.model = model
        return prepare

    dense = C.run_model("wan-D128", dtype, "cuda", dtype)
    for w in (C.WAN_GRID[0] - 1, 100):
        prep = window(w)
        out = C.run_model("wan-D128", dtype, "cuda", dtype, prepare=prep)
        assert not prep.model._mask_cache
        assert torch.equal(out, dense), w
    assert "attn_fwd_bshd_masked/block" not in entry_counts
    prep = window(1)
    out = C.run_model("wan-D128", dtype, "cuda", dtype, prepare=prep)
    assert len(prep.model._mask_cache) == 1
    assert entry_counts["attn_fwd_bshd_masked/block"] == 2      # depth 2
    assert not torch.equal(out, dense)


@DTYPES
@pytest.mark.parametrize("case", [
    C.CASES[0], C.cases("single")[0], C.cases("wan")[1], C.cases("last")[0],
    C.cases("sdtx")[0], C.cases("res")[0]], ids=lambda c: c.id)
def test_two_calls_are_bit_identical(case, dtype, no_fallback):
    built = C.build(case, dtype)
    a = C.run(built, "cuda", dtype)
    b = C.run(built, "cuda", dtype)
    for tap in a:
        assert torch.equal(a[tap], b[tap]), tap


# ---------------- c. GPU-only branches in fp32 ----------------

@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_fp32_blocks(case):
    """fp32 on the GPU: attention takes the reference path, the norms their
    fp32 kernels, GELULinear its _addmm_activation epilogue, SingleStream
    the addmm accumulate, the bank its slices. Limit per tap: M32 * the CPU
    fp32 run's distance from fp64; erf-for-tanh GELU exceeds twice that
    (test_block_cases_reference)."""
    built = C.build(case, C.BF16)
    ref, e_ref = C.reference(built), C.e_ref(built, C.F32)
    e_gpu = C.errors(C.run(built, "cuda", C.F32), ref)
    _report(f"{case.id} fp32", e_gpu, e_ref)
    for tap, e in e_gpu.items():
        assert e <= C.M32 * e_ref[tap], (
            f"{case.kind} block, case {case.id} fp32: tap {tap} is {e:.3e} "
            f"from fp64, limit {C.M32} x {e_ref[tap]:.3e}")


# ---------------- d. whole models at a real head dim ----------------

@DTYPES
@pytest.mark.parametrize("name", list(C.MODEL_CASES))
def test_whole_model_against_fp64(name, dtype, no_fallback, entry_counts):
    """One masked forward per family at head dim 64 / 128 and the blocks'
    sequence, against the same weights in fp64 on the CPU; the limit is
    M_MODEL * the CPU 16-bit forward's own distance from fp64."""
    ref = C.model_reference(name, dtype)
    e_ref = C.model_e_ref(name, dtype)
    out = C.run_model(name, dtype, "cuda", dtype)
    e_gpu = C.rel_l2(out, ref)
    print(f"\n{name} {DT_IDS[dtype]}: {e_gpu:.3e}/{e_ref:.3e}"
          f"={e_gpu / e_ref:.3f}  {entry_counts}")
    want = {
        "flux": {"attn_fwd_bshd_split_masked/key": 2,
                 "attn_fwd_bshd_masked/key": 2, "pack_joint_qkv": 2,
                 "qk_norm_rope_": 2, "layer_norm_mod": 11,
                 "gate_residual": 10},
        "sd3": {"attn_fwd_bshd_split_masked/key": 2, "pack_joint_qkv": 2,
                "layer_norm_mod": 9, "gate_residual": 8},
        "zimage": {"attn_fwd_bshd_masked/key": 2, "qk_norm_rope_": 2,
                   "layer_norm_mod": 3, "gate_residual": 2},
        "wan-D128-win1": {"attn_fwd_bshd_masked/block": 2,
                          "attn_fwd_bshd_masked/key": 2, "qk_norm_rope_": 2,
                          "layer_norm_mod": 5, "gate_residual": 4},
        "wan": {"attn_fwd_bshd": 2, "attn_fwd_bshd_masked/key": 2,
                "qk_norm_rope_": 2, "layer_norm_mod": 5, "gate_residual": 4},
        # 7 SpatialTransformers of depth 1: self + cross each
        "sd15": {"attn_fwd_bshd": 7, "attn_fwd_bshd_masked/key": 7,
                 "group_norm_silu": 17},
    }
    key = name if name in want else name.split("-")[0]
    assert entry_counts == want[key], (name, entry_counts)
    assert e_gpu <= C.M_MODEL[dtype] * e_ref, (
        f"{name} {DT_IDS[dtype]}: {e_gpu:.3e} from fp64, limit "
        f"{C.M_MODEL[dtype]} x {e_ref:.3e} (ratio {e_gpu / e_ref:.3f})")
