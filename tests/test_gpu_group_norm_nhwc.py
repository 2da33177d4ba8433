"""The channels-last GroupNorm kernels (ops/hip/group_norm_nhwc.h) and the
channels-last UNet mode on the GPU.

Shapes (B, C, H, W, G) are the smallest that reach each path: a vector that
spans two groups (10 channels per group) and four (C = 8, G = 4), two
columns per thread (C = 2560), many automatic slabs with a ragged last one
(67 x 67), one pixel; forced slabs of 1, 4 and more than HW pixels. The
comparison, the rows and the tolerances are test_group_norm_channels_last's
(group_norm_cases.py).
"""
import copy
import logging

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models import sd_unet as U
from comfyui_parallelanything_amd.models.registry import MODELS
from comfyui_parallelanything_amd.ops import reference as R
from group_norm_cases import (CL, check_rows, group_norm_f64, is_cl,
                              refusals, run_regimes)

SHAPES = ((2, 40, 5, 7, 4), (1, 8, 3, 3, 4), (1, 2560, 3, 3, 32),
          (1, 40, 67, 67, 4), (3, 64, 1, 1, 32))
SHAPE_IDS = ("cpg10", "c8g4", "c2560", "slabs67", "px1")
DT16 = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
TOL = C.TOL_GN


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available("group_norm_nhwc"), (
        "native _pa_hip extension must be present on a GPU box")


@pytest.fixture()
def no_fallback(monkeypatch):
    seen = []
    orig = ops._unsupported

    def spy(op, why):
        seen.append((op, why))
        return orig(op, why)

    monkeypatch.setattr(ops, "_unsupported", spy)
    yield seen
    assert not seen, f"ops fell back to the reference path: {seen}"


def _op(x, G, w, b, eps, silu, add):
    return ops.group_norm(x, G, w, b, eps, silu=silu, channel_add=add)


def _forced(slab_pixels):
    ext = ops.hip_ext()

    def call(x, G, w, b, eps, silu, add):
        return ext.group_norm_nhwc(x, G, w, b, add, eps, silu, slab_pixels)
    return call


def _case(shape, dtype, seed=11):
    """x channels-last, w, b, add on the GPU, and the CPU originals."""
    B, Cn, H, W, G = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (3.0 + 2.0 * torch.randn(B, Cn, H, W, generator=g)).to(dtype)
    w = torch.randn(Cn, generator=g).to(dtype)
    b = torch.randn(Cn, generator=g).to(dtype)
    add = torch.randn(B, Cn, generator=g).to(dtype)
    cpu = (x, w, b, add)
    return [x.contiguous(memory_format=CL).cuda(), w.cuda(), b.cuda(),
            add.cuda()], cpu, G


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@DT16
def test_group_norm_against_fp64(dtype, shape, no_fallback):
    run_regimes(shape, dtype, _op, device="cuda")


@pytest.mark.parametrize("slab_pixels", [1, 4, 1000])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=SHAPE_IDS[:2])
@DT16
def test_forced_slabs(dtype, shape, slab_pixels):
    run_regimes(shape, dtype, _forced(slab_pixels), device="cuda")


@DT16
def test_statistics_are_per_batch_element(dtype, no_fallback):
    """Three batch elements six decades apart, and an addend that differs
    per batch element: statistics leaking across b would be far off."""
    (x, w, b, add), (xc, wc, bc, addc), G = _case((3, 40, 5, 7, 4), dtype)
    scale = torch.tensor([1e-2, 1.0, 1e2])
    xc = (xc.float() * scale[:, None, None, None]).to(dtype)
    addc = (addc.float() * scale[:, None] * 3.0).to(dtype)
    x = xc.contiguous(memory_format=CL).cuda()
    out = ops.group_norm(x, G, w, b, 1e-6, silu=True, channel_add=addc.cuda())
    ref = group_norm_f64(xc, G, wc, bc, 1e-6, True, addc)
    check_rows(out, ref, G, dtype, "plain", TOL, "per-batch")
    # and each batch element alone gives the same bits
    for i in range(3):
        one = ops.group_norm(x[i:i + 1], G, w, b, 1e-6, silu=True,
                             channel_add=addc[i:i + 1].cuda())
        assert torch.equal(one, out[i:i + 1]), i


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@DT16
def test_repeatable_inputs_untouched_output_format(dtype, shape, no_fallback):
    (x, w, b, add), _, G = _case(shape, dtype)
    x0, add0, w0, b0 = x.clone(), add.clone(), w.clone(), b.clone()
    y1 = ops.group_norm(x, G, w, b, silu=True, channel_add=add)
    y2 = ops.group_norm(x, G, w, b, silu=True, channel_add=add)
    assert torch.equal(y1, y2)
    for t, t0 in ((x, x0), (add, add0), (w, w0), (b, b0)):
        assert torch.equal(t, t0), "an input was modified"
    assert y1.shape == x.shape and y1.dtype == dtype and is_cl(y1)
    assert y1.stride() == x.stride()
    B, Cn, H, W = x.shape
    tok = y1.permute(0, 2, 3, 1).reshape(B, H * W, Cn)
    assert tok.data_ptr() == y1.data_ptr()


def test_empty_input():
    for shape in ((0, 16, 4, 4), (2, 16, 0, 4), (2, 16, 4, 0)):
        x = torch.empty(shape, device="cuda", dtype=C.BF16).contiguous(
            memory_format=CL)
        y = ops.group_norm(x, 4, silu=True)
        assert y.shape == x.shape and y.dtype == x.dtype


@DT16
def test_graph_capture(dtype):
    (x, w, b, add), _, G = _case((2, 40, 5, 7, 4), dtype)
    eager = ops.group_norm(x, G, w, b, silu=True, channel_add=add)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.group_norm(x, G, w, b, silu=True, channel_add=add)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.group_norm(x, G, w, b, silu=True, channel_add=add)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)


def test_offsets_past_2_31():
    """Batch element 1 of a two-element x spans element offsets 2^30 + 2^26
    to 2^31 + 2^27: its result must be bit for bit that of the same data at
    offset 0. The smallest x that reaches such an offset is 4.6 GB, and the
    op needs as much again for its result: about 12 GB at the peak here,
    freed as it goes, and skipped where the card does not have them free."""
    B, Cn, H, W, G = 2, 8, 8192, 16384 + 1024, 4
    if torch.cuda.mem_get_info()[0] < 16 << 30:
        pytest.skip("less than 16 GiB free on the device")
    x = torch.empty(B, H, W, Cn, device="cuda", dtype=C.BF16)
    x[0].zero_()
    g = torch.Generator(device="cuda").manual_seed(3)
    x[1].normal_(1.0, 2.0, generator=g)
    x = x.permute(0, 3, 1, 2)
    assert is_cl(x) and x[0].numel() < 2 ** 31 < x.numel()
    ext = ops.hip_ext()
    npx = 1 << 17
    one = ext.group_norm_nhwc(x[1:2], G, None, None, None, 1e-6, True, npx)
    big = ext.group_norm_nhwc(x, G, None, None, None, 1e-6, True, npx)
    assert torch.equal(big[1:2], one)
    assert not big[0].any()
    del big
    # and that result is a GroupNorm: the first and last pixels against fp64
    tok = x[1].permute(1, 2, 0).reshape(-1, Cn)          # [HW, C], a view
    got = one[0].permute(1, 2, 0).reshape(-1, Cn)
    cpg = Cn // G
    for gi in range(G):
        cols = slice(gi * cpg, (gi + 1) * cpg)
        var, mean = torch.var_mean(tok[:, cols].float(), correction=0)
        for rows in (slice(0, 64), slice(-64, None)):
            ref = ((tok[rows, cols].double() - mean.double())
                   * torch.rsqrt(var.double() + 1e-6))
            C.check(got[rows, cols], ref * torch.sigmoid(ref), *TOL,
                    what=f"2^31, group {gi}")


# ---------------- launcher refusals, dispatch ----------------

def _launcher_refusals():
    ext = ops.hip_ext()
    x = torch.randn(2, 16, 3, 3, device="cuda", dtype=C.BF16).contiguous(
        memory_format=CL)
    v = torch.ones(16, device="cuda", dtype=C.BF16)
    a = torch.ones(2, 16, device="cuda", dtype=C.BF16)

    def call(x_, G=4, w=None, b=None, add=None):
        return ext.group_norm_nhwc(x_, G, w, b, add, 1e-6, False, 0)

    yield "x on the CPU", lambda: call(x.cpu())
    yield "x NCHW", lambda: call(x.contiguous())
    yield "x a strided slice", lambda: call(x[:, :, :, ::2])
    yield "x 3-D", lambda: call(x[0])
    yield "C % groups", lambda: call(x, 5)
    yield "C % 8", lambda: call(x[:, :12].contiguous(memory_format=CL), 4)
    yield "fp32 x", lambda: call(x.float())
    yield "weight on the CPU", lambda: call(x, 4, v.cpu(), v)
    yield "bias on the CPU", lambda: call(x, 4, v, v.cpu())
    yield "add on the CPU", lambda: call(x, 4, add=a.cpu())
    for what, args, kw in refusals("cuda", C.BF16):
        if what == "x is 3-D":
            continue
        yield what, lambda args=args, kw=kw: call(
            args[0], args[1], *(args[2:] or (None, None)),
            kw.get("channel_add"))


def test_launcher_refusals_leave_the_next_call_right():
    (x, w, b, add), (xc, wc, bc, addc), G = _case((2, 40, 5, 7, 4), C.BF16)
    ref = group_norm_f64(xc, G, wc, bc, 1e-6, False, addc)
    n = 0
    for what, bad in _launcher_refusals():
        with pytest.raises(RuntimeError):
            bad()
        n += 1
        out = ops.group_norm(x, G, w, b, channel_add=add)
        C.check(out, ref, *TOL, what=f"after '{what}'")
    assert n >= 19


def test_op_refusals_raise_on_the_gpu():
    for what, args, kw in refusals("cuda", C.BF16):
        with pytest.raises(RuntimeError, match="group_norm"):
            ops.group_norm(*args, **kw)
    x = torch.randn(1, 8, 2, 2, device="cuda", dtype=C.BF16)
    with pytest.raises(RuntimeError, match="is on"):
        ops.group_norm(x, 4, torch.ones(8, dtype=C.BF16),
                       torch.ones(8, dtype=C.BF16))


@DT16
def test_nchw_input_warns_once_and_matches_reference(dtype, caplog):
    g = torch.Generator(device="cpu").manual_seed(2)
    x = torch.randn(2, 16, 5, 3, generator=g).to(dtype).cuda()
    w = torch.randn(16, generator=g).to(dtype).cuda()
    b = torch.randn(16, generator=g).to(dtype).cuda()
    assert x.is_contiguous() and not is_cl(x)
    ops._WARNED.discard(("group_norm", "not dense channels-last"))
    with caplog.at_level(logging.WARNING, logger="parallelanything.ops"):
        y1 = ops.group_norm(x, 4, w, b, silu=True)
        y2 = ops.group_norm(x, 4, w, b, silu=True)
    said = [r for r in caplog.records if "group_norm" in r.getMessage()]
    assert len(said) == 1, [r.getMessage() for r in said]
    assert y1.is_contiguous() and y1.dtype == dtype
    assert torch.equal(y1, R.group_norm(x, 4, w, b, silu=True))
    assert torch.equal(y1, y2)
    # fp32 and C % 8 != 0 go the same way
    for t, G in ((x.float().contiguous(memory_format=CL), 4),
                 (x[:, :12].contiguous(memory_format=CL), 4)):
        y = ops.group_norm(t, G)
        assert torch.equal(y, R.group_norm(t, G)) and is_cl(y)


# ---------------- models ----------------

# tests/test_gpu_kernels.py::test_whole_model_gpu_vs_cpu_reference and
# tests/test_gpu_fp16.py::test_whole_model_fp16_gpu_vs_cpu_reference: the
# 16-bit native forward against the fp32 CPU forward of the same weights
WHOLE_MODEL_REL_L2 = 0.15
WHOLE_MODEL_CORR = 0.99


@pytest.mark.parametrize("name", ["sd15", "sdxl"])
@DT16
def test_channels_last_whole_model(dtype, name, no_fallback):
    make, inputs = MODELS[name]
    m_ref = make(dev="cpu", dtype=torch.float32, tiny=True)
    m_gpu = copy.deepcopy(m_ref).to_channels_last().to("cuda", dtype)
    assert all(is_cl(p.weight) for p in m_gpu.modules()
               if isinstance(p, torch.nn.Conv2d))
    x, t, c, kw = inputs(2, tiny=True, dtype=torch.float32)
    seen = []
    for mod in m_gpu.modules():
        if isinstance(mod, (U.GNSiLU, U.SpatialTransformer)):
            mod.register_forward_pre_hook(
                lambda mod, args: seen.append(is_cl(args[0])))
    with torch.no_grad():
        ref = m_ref(x, t, context=c, **kw).float()
        out = m_gpu(
            x.cuda().to(dtype), t.cuda(), context=c.cuda().to(dtype),
            **{k: (v.cuda().to(dtype) if isinstance(v, torch.Tensor) else v)
               for k, v in kw.items()})
    assert out.dtype == dtype and out.is_contiguous() and out.shape[1] == 4
    assert seen and all(seen), "an activation left channels-last"
    out = out.float().cpu()
    rel = ((out - ref).norm() / ref.norm()).item()
    corr = torch.corrcoef(
        torch.stack([out.flatten(), ref.flatten()]))[0, 1].item()
    print(f"{name}: channels-last whole-model rel-l2 {rel:.5f} "
          f"corr {corr:.6f}")
    assert rel < WHOLE_MODEL_REL_L2, f"{name}: whole-model rel-l2 {rel:.4f}"
    assert corr > WHOLE_MODEL_CORR, f"{name}: correlation {corr:.4f}"


@pytest.fixture()
def entry_counts(monkeypatch):
    """test_gpu_blocks.py's pattern, for the two GroupNorm entry points."""
    ext = ops.hip_ext()
    counts = {}

    def wrap(name, fn):
        def counted(*args):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args)
        return counted

    for name in ("group_norm_nhwc", "group_norm_silu"):
        monkeypatch.setattr(ext, name, wrap(name, getattr(ext, name)))
    return counts


@pytest.mark.parametrize("channels_last", [True, False],
                         ids=["channels_last", "default"])
def test_resblock_entry_points(channels_last, entry_counts, no_fallback):
    torch.manual_seed(4)
    blk = U.ResBlock(32, 64, 128).cuda().to(C.BF16).eval()
    x = torch.randn(2, 32, 6, 5, device="cuda", dtype=C.BF16)
    emb = torch.randn(2, 128, device="cuda", dtype=C.BF16)
    with torch.no_grad():
        ref = blk(x, emb)
        assert entry_counts == {"group_norm_silu": 2}
        if not channels_last:
            return
        entry_counts.clear()
        for m in blk.modules():
            if isinstance(m, (U.GNSiLU, U.ResBlock)):
                m.channels_last = True
        out = blk(x.contiguous(memory_format=CL), emb)
    assert entry_counts == {"group_norm_nhwc": 2}, entry_counts
    assert is_cl(out)
    C.check(out, ref.float(), 3e-2, 3e-2, what="channels-last ResBlock")
