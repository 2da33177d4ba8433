"""Shared by test_group_norm_channels_last.py (CPU) and
test_gpu_group_norm_nhwc.py (GPU): the fp64 GroupNorm with the addend, the
row comparison with group_norm_silu's constant-row policy, the walk over
kernel_cases.NORM_RUNS x options, and the calls the op refuses."""
import itertools

import torch

import kernel_cases as C

CL = torch.channels_last
F32 = torch.float32
OPTIONS = list(itertools.product((False, True), repeat=3))  # silu, affine, add


def is_cl(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=CL)


def group_norm_f64(x, G, w=None, b=None, eps=1e-6, silu=False, add=None):
    """GroupNorm in fp64 of the op's input: x, or with an addend the fp32
    sum x + add, which is the contract (the addend joins in fp32 and that
    sum is not rounded to x's dtype). An exact sum would ask the op for
    digits fp32 does not have: 1e15 + 0.3 is 1e15."""
    xd = x.double()
    if add is not None:
        xd = (x.float() + add.float()[:, :, None, None]).double()
    B = xd.shape[0]
    out = C.layer_norm_f64(xd.reshape(B, G, -1), eps).reshape(xd.shape)
    if w is not None:
        out = out * w.double()[None, :, None, None]
    if b is not None:
        out = out + b.double()[None, :, None, None]
    return out * torch.sigmoid(out) if silu else out


def check_rows(out, ref, G, dtype, regime, tol, what):
    """Finite everywhere; close to fp64 on every (b, g) row, but on constant
    rows only for the constants group_norm_silu compares (kernel_cases.
    compared_constant). The policy holds with an addend too: a group of c +
    a_i deviates by the addend alone, as little as two of its values are
    close, and the fp32 reference path, which runs this same comparison on
    the CPU, holds its mean to 2^-24 c at best."""
    out = out.cpu()
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
    B = out.shape[0]
    o = out.reshape(B * G, -1)
    r = ref.reshape(B * G, -1)
    rows = list(range(B * G))
    if regime == "constant":
        rows = [i for i in rows
                if C.compared_constant("group_norm_silu", dtype, i)]
    C.check(o[rows], r[rows], *tol, what=what)


def run_regimes(shape, dtype, call, device="cpu"):
    """Every (regime, eps) of NORM_RUNS x silu x affine x channel_add at one
    shape: call(x, G, w, b, eps, silu, add) -> out, x channels-last."""
    tol = C.norm_tol(dtype, C.TOL_GN)
    for regime, eps in C.NORM_RUNS:
        x, w, b, G = C.group_norm_case(regime, shape, dtype)
        add = C.plain(x.shape[0], x.shape[1], dtype, 9)
        xc = x.contiguous(memory_format=CL).to(device)
        for silu, affine, with_add in OPTIONS:
            a = add if with_add else None
            wb = (w, b) if affine else (None, None)
            out = call(xc, G, *(None if t is None else t.to(device)
                                for t in wb), eps, silu,
                       None if a is None else a.to(device))
            what = (f"{regime} eps={eps} silu={silu} affine={affine} "
                    f"add={with_add}")
            assert out.dtype == dtype and out.shape == x.shape, what
            assert is_cl(out), f"{what}: output is not channels-last"
            ref = group_norm_f64(x, G, *wb, eps, silu, a)
            check_rows(out, ref, G, dtype, regime, tol, what)


def refusals(dev="cpu", dtype=F32):
    """(what, args, kwargs) of every call the op refuses on every device."""
    other = torch.float64 if dtype == F32 else (
        C.F16 if dtype == C.BF16 else C.BF16)
    x = torch.randn(2, 16, 3, 3, device=dev).to(dtype).contiguous(
        memory_format=CL)
    v = torch.ones(16, device=dev, dtype=dtype)
    a = torch.ones(2, 16, device=dev, dtype=dtype)
    yield "x is 3-D", (x[0], 4), {}
    yield "C % groups", (x, 5), {}
    yield "weight dtype", (x, 4, v.to(other), v), {}
    yield "bias dtype", (x, 4, v, v.to(other)), {}
    yield "add dtype", (x, 4), {"channel_add": a.to(other)}
    yield "weight shape", (x, 4, v[:8], v), {}
    yield "weight 2-D", (x, 4, v[None], v), {}
    yield "bias shape", (x, 4, v, torch.ones(17, device=dev, dtype=dtype)), {}
    yield "add shape", (x, 4), {"channel_add": a[:1]}
    yield "add 1-D", (x, 4), {"channel_add": v}
    yield "add strided", (x, 4), {
        "channel_add": torch.ones(16, 2, device=dev, dtype=dtype).t()}
