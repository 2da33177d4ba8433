"""Native gfx950 norm kernels and GELU on rows that are not N(0,1).

test_gpu_kernels.py and test_gpu_fp16.py feed randn: mean 0, variance 1, no
outlier, default eps. Here the rows are tiny (variance ~ eps), offset (mean
40), carry one outlier of 500, are constant, or huge, and eps is also passed
as 1e-2 and 1e-5 (kernel_cases.py; test_kernel_cases_reference.py shows on
the CPU that these rows reject an ignored or misplaced eps, a skipped mean, a
skipped last vector and an unclamped variance). References are fp64, written
out in kernel_cases.py; tolerances are test_gpu_kernels.py's per op.

Shapes are the smallest that reach each path: rms_norm's one-wave-per-row
kernel at its limits (D=128, D=512, 5 rows for the 4-rows-per-block tail),
the vector kernels with 1, 257 and 640 vectors per row (D=8, 2056, 5120),
the scalar kernels (D=20, and every fp32 input).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

F32 = torch.float32
DT16 = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DT = pytest.mark.parametrize("dtype", C.DTYPES + (F32,),
                             ids=C.DTYPE_IDS + ("fp32",))


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available(), (
        "native _pa_hip extension must be present on a GPU box"
    )


def _check_rows(out, ref, op, dtype, regime, tol, what):
    """out / ref [rows, ...]: finite everywhere; close to fp64 on every row,
    but on constant rows only for the constants kernel_cases.py compares."""
    out = out.cpu()
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
    rows = list(range(out.shape[0]))
    if regime == "constant":
        rows = [i for i in rows if C.compared_constant(op, dtype, i)]
        assert 2 * len(rows) >= out.shape[0] or dtype == F32
    C.check(out[rows], ref[rows], *tol, what=what)


@pytest.mark.parametrize("rows,D", C.RMS_SHAPES)
@DT
def test_rms_norm_regimes(dtype, rows, D):
    tol = C.norm_tol(dtype, C.TOL_RMS)
    w = C.plain(1, D, dtype, 5)[0]
    for regime, eps in C.NORM_RUNS:
        n = C.CONSTANT_ROWS if regime == "constant" else rows
        x = C.norm_rows(regime, n, D, dtype, D)
        out = ops.rms_norm(x.cuda(), w.cuda(), eps)
        assert out.dtype == dtype
        _check_rows(out, C.rms_norm_f64(x, w, eps), "rms_norm", dtype, regime,
                    tol, f"{regime} eps={eps}")
    x = C.norm_rows("offset", rows, D, dtype, D)
    _check_rows(ops.rms_norm(x.cuda(), None), C.rms_norm_f64(x), "rms_norm",
                dtype, "offset", tol, "no weight")


@pytest.mark.parametrize("D", C.LN_DIMS)
@DT
def test_layer_norm_mod_regimes(dtype, D):
    tol = C.norm_tol(dtype, C.TOL_LN)
    sc, sh = C.modulation(2, D, dtype, 6)
    for regime, eps in C.NORM_RUNS:
        n = C.CONSTANT_ROWS if regime == "constant" else 6
        x = C.norm_rows(regime, n, D, dtype, D).view(2, n // 2, D)
        out = ops.layer_norm_mod(x.cuda(), sc.cuda(), sh.cuda(), eps)
        assert out.dtype == dtype
        ref = C.layer_norm_mod_f64(x, sc, sh, eps)
        _check_rows(out.view(n, D), ref.view(n, D), "layer_norm_mod", dtype,
                    regime, tol, f"{regime} eps={eps}")


@pytest.mark.parametrize("shape", C.GN_SHAPES, ids=["n18", "n280", "cpg1"])
@DT
def test_group_norm_silu_regimes(dtype, shape):
    tol = C.norm_tol(dtype, C.TOL_GN)
    for regime, eps in C.NORM_RUNS:
        x, w, b, G = C.group_norm_case(regime, shape, dtype)
        out = ops.group_norm_silu(x.cuda(), G, w.cuda(), b.cuda(), eps)
        assert out.dtype == dtype and out.shape == x.shape
        rows = x.shape[0] * G
        ref = C.group_norm_silu_f64(x, G, w, b, eps)
        _check_rows(out.reshape(rows, -1), ref.reshape(rows, -1),
                    "group_norm_silu", dtype, regime, tol,
                    f"{regime} eps={eps}")
    x, _, _, G = C.group_norm_case("offset", shape, dtype)
    out = ops.group_norm_silu(x.cuda(), G, None, None)
    C.check(out, C.group_norm_silu_f64(x, G), *tol, what="no affine")


def _qkv_from_rows(rows, B, S, H, D):
    """[B, S, 3, H, D] whose q rows are rows[:B*S*H], k rows the next B*S*H
    and v rows the ones after, each in (b, s, h) order."""
    n = B * S * H
    return torch.stack([rows[j * n:(j + 1) * n].view(B, S, H, D)
                        for j in range(3)], dim=2).contiguous()


def _constant_offsets(regime, step):
    """Constant rows: two calls, so that the q and k rows of both together
    hold every one of the 32 constants."""
    return (0, step) if regime == "constant" else (0,)


@pytest.mark.parametrize("D", C.QK_DIMS)
@DT16
def test_qk_norm_rope_regimes(dtype, D):
    B, S, H = 1, 3, 3                    # 9 rows: the 4-rows-per-wave tail
    n = B * S * H
    wq = C.plain(1, D, dtype, 21)[0]
    wk = C.plain(1, D, dtype, 22)[0]
    cs = R.rope_freqs(torch.arange(S), D)
    for regime, eps in C.NORM_RUNS:
        for lo in _constant_offsets(regime, 14):
            rows = C.norm_rows(regime, lo + 3 * n, D, dtype, D)[lo:]
            qkv = _qkv_from_rows(rows, B, S, H, D)
            dev = qkv.clone().cuda()
            q, k, v = dev.unbind(2)
            ops.qk_norm_rope_(q, k, wq.cuda(), wk.cuda(), cs.cuda(), eps)
            what = f"{regime} eps={eps} rows {lo}.."
            for name, got, j, w in (("q", q, 0, wq), ("k", k, 1, wk)):
                assert torch.isfinite(got.float()).all(), f"{what} {name}"
                C.check(got, C.qk_norm_rope_f64(qkv[:, :, j], w, cs, eps),
                        *C.TOL_QK, what=f"{what} {name}")
            assert torch.equal(v.cpu(), qkv[:, :, 2]), f"{what}: v modified"


@pytest.mark.parametrize("D", C.QK_DIMS)
@DT16
def test_pack_joint_qkv_regimes(dtype, D):
    B, T, Si, H = 1, 2, 3, 3
    nt, ni = B * T * H, B * Si * H
    ws = [C.plain(1, D, dtype, 23 + i)[0] for i in range(4)]
    cs = R.rope_freqs(torch.arange(T + Si), D)
    for regime, eps in C.NORM_RUNS:
        for lo in _constant_offsets(regime, 12):
            rows = C.norm_rows(regime, lo + 3 * (nt + ni), D, dtype, D)[lo:]
            txt = _qkv_from_rows(rows[:3 * nt], B, T, H, D)
            img = _qkv_from_rows(rows[3 * nt:], B, Si, H, D)
            q, k, v = ops.pack_joint_qkv(
                txt.clone().cuda(), img.clone().cuda(),
                *(w.cuda() for w in ws), cs.cuda(), eps)
            what = f"{regime} eps={eps} rows {lo}.."
            for name, got, j in (("q", q, 0), ("k", k, 1)):
                ref = torch.cat([
                    C.qk_norm_rope_f64(txt[:, :, j], ws[j], cs[:T], eps),
                    C.qk_norm_rope_f64(img[:, :, j], ws[2 + j], cs[T:], eps)],
                    dim=1)
                assert torch.isfinite(got.float()).all(), f"{what} {name}"
                C.check(got, ref, *C.TOL_QK, what=f"{what} {name}")
            assert torch.equal(
                v.cpu(), torch.cat([txt[:, :, 2], img[:, :, 2]], dim=1)), what


@pytest.mark.parametrize("D", [8, 3072, 5120])
def test_layer_norm_mod_fp8_degenerate_rows(D):
    """Constant and offset rows through the fused LayerNorm + e4m3 cast: a
    NaN rstd would poison the output and, through amax, every later scale."""
    assert ops.hip_available("layer_norm_mod_fp8")
    sc, sh = C.modulation(2, D, C.BF16, 6)
    for regime in ("constant", "offset"):
        n = C.CONSTANT_ROWS if regime == "constant" else 6
        x = C.norm_rows(regime, n, D, C.BF16, D).view(2, n // 2, D)
        qscale = torch.ones(1, device="cuda")
        amax = torch.zeros(2, device="cuda")
        used = torch.zeros(1, device="cuda")
        x8 = ops.layer_norm_mod_fp8(x.cuda(), sc.cuda(), sh.cuda(), qscale,
                                    amax, used)
        assert x8.dtype == torch.float8_e4m3fn
        assert torch.isfinite(x8.float()).all(), regime
        assert torch.isfinite(amax).all() and torch.isfinite(qscale).all()
        ref = C.layer_norm_mod_f64(x, sc, sh)
        want = ref.abs().amax().item()
        assert abs(amax[0].item() - want * 0.999) <= 5e-2 * want, \
            f"{regime}: amax {amax[0].item()} for a true {want}"


@pytest.mark.parametrize("path", ["vector", "strided_slice", "w6", "numel17"])
@DT16
def test_gelu_tanh_special_values(dtype, path):
    """+-0, the linear range, saturation, the largest finite inputs (whose
    cube overflows fp32 for bf16), +-inf and NaN, through the vector kernel,
    the strided-slice form of it, and the two exits for widths that are no
    multiple of 8."""
    vals = C.gelu_values(dtype).cuda()
    n = vals.numel()
    if path == "vector":
        x = vals.repeat(3, 1)                            # [3, n], n % 8 == 0
    elif path == "strided_slice":
        big = torch.full((3, n + 24), 0.25, dtype=dtype, device="cuda")
        big[:, 16:16 + n] = vals
        x = big[:, 16:16 + n]
        assert not x.is_contiguous()
    elif path == "w6":
        x = vals.view(n // 6, 6)                         # w % 8 != 0, one row
    else:
        x = vals[:17].clone()                            # numel % 8 != 0
    out = ops.gelu_tanh(x)
    assert out.shape == x.shape and out.dtype == dtype
    ref = F.gelu(x.float().cpu(), approximate="tanh")
    C.check(out, ref, *C.TOL_GELU, what=path, equal_nan=True)
    # no NaN but where the reference has one (NaN itself and 0 * -inf)
    assert torch.equal(out.float().isnan().cpu(), ref.isnan())
