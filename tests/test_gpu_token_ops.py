"""The UNet token kernels (ops/hip/token_ops.h) on the GPU. Bound per element:
0.5 * spacing16(ref) + 2 * k_ref * term, term one fp32 rounding of the op's
largest intermediate and k_ref the distance from fp64, in terms, of the same
fp32 arithmetic on the CPU, same inputs. docs/KERNELS.md, "UNet token ops"."""
import logging

import pytest
import torch
import torch.nn.functional as F

import kernel_cases as C
from comfyui_parallelanything_amd import ops

pytestmark = pytest.mark.gpu

DT16 = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
EPS32 = 2.0 ** -24


@pytest.fixture()
def no_fallback(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "_unsupported", lambda *a: seen.append(a))
    yield seen
    assert not seen, f"ops fell back to the reference path: {seen}"


def check_bound(out, ref, r32, term, what):
    fi = torch.finfo(out.dtype)
    half = 0.5 * fi.eps * torch.exp2(torch.floor(torch.log2(
        ref.abs().clamp_min(fi.tiny))))         # half a 16-bit spacing at ref
    term = term.clamp_min(1e-300)
    k_ref = ((r32.double() - ref).abs() / term).max().item()
    k = (((out.double().cpu() - ref).abs() - half) / term).max().item()
    print(f"{what}: k = {k:.3f}, k_ref = {k_ref:.3f}")
    assert k <= 2.0 * k_ref, f"{what}: k = {k:.3f} > 2 * {k_ref:.3f}"


def ln_inputs(kind, rows, D, dtype):
    # x, delta (zero where the sum must stay constant), weight, bias
    g = torch.Generator().manual_seed(rows * D)
    x, delta, w, b = torch.randn(4, rows, D, generator=g)
    if kind in ("offset300", "zeros"):
        x = (300.0 + 0.1 * x if kind == "offset300" else 0.0 * x).to(dtype)
    else:
        x = C.norm_rows(kind, rows, D, dtype, seed=D)
    delta = delta * (0.0 if kind in ("constant", "zeros") else 0.5)
    return x, delta.to(dtype), w[0].to(dtype), b[0].to(dtype)


@pytest.mark.parametrize("kind", ["plain", "offset300", "constant", "zeros",
                                  "tiny", "offset", "outlier", "huge"])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", [(1, 8), (5, 320), (7, 520), (3, 1280),
                                   (6, 2048)], ids=lambda s: f"{s[0]}x{s[1]}")
@DT16
def test_layer_norm_against_fp64(dtype, shape, residual, kind, no_fallback):
    x, delta, w, b = ln_inputs(kind, *shape, dtype)
    s = (x.float() + delta.float()).to(dtype) if residual else x
    xg, dg, wg, bg = (t.cuda() for t in (x, delta, w, b))
    for eps in (1e-5, 1e-6):
        if residual:
            s_out, y = ops.layer_norm(dg, wg, bg, eps, residual=xg)
            assert torch.equal(s_out.cpu(), s) and torch.equal(
                y, ops.layer_norm(s_out, wg, bg, eps))
        else:
            y = ops.layer_norm(xg, wg, bg, eps)
        sd, wd, bd = s.double(), w.double(), b.double()
        rstd = torch.rsqrt(sd.var(-1, unbiased=False, keepdim=True) + eps)
        check_bound(
            y, F.layer_norm(sd, sd.shape[-1:], wd, bd, eps),
            F.layer_norm(s.float(), s.shape[-1:], w.float(), b.float(), eps),
            EPS32 * (wd.abs() * rstd * sd.abs().amax(-1, keepdim=True)
                     + bd.abs()), f"layer_norm {kind} eps={eps}")


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("rows, N", [(1, 8), (5, 40), (3, 2560)])
@DT16
def test_geglu_against_fp64(dtype, rows, N, sliced, no_fallback):
    torch.manual_seed(N)
    a = torch.randn(rows, N).to(dtype)
    gate = torch.linspace(-12, 12, rows * N).reshape(rows, N).to(dtype)
    y = torch.cat([a, gate], -1).cuda()
    if sliced:      # a column slice of a wider buffer: row stride 2N + 24
        wide = torch.full((rows, 2 * N + 24), float("nan"), device="cuda",
                          dtype=dtype)
        wide[:, 8:-16] = y
        y = wide[:, 8:-16]
    kept = y.clone()
    out = ops.geglu(y)
    assert out.is_contiguous() and torch.equal(out, ops.geglu(y))
    assert torch.equal(y, kept), "input touched"
    check_bound(out, a.double() * F.gelu(gate.double()),
                a.float() * F.gelu(gate.float()),
                EPS32 * (a.double() * gate.double()).abs(), "geglu")


@DT16
def test_exact_properties_and_graph_capture(dtype, no_fallback):
    x, delta, w, b = (t.cuda() for t in ln_inputs("plain", 5, 528, dtype))
    kept = [t.clone() for t in (x, delta, w, b)]

    def both():
        s, y = ops.layer_norm(delta, w, b, residual=x)
        return s, y, ops.geglu(y)
    eager = both()
    assert all(torch.equal(o, e) for o, e in zip(both(), eager))
    assert all(torch.equal(a, k) for a, k in zip((x, delta, w, b), kept))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = both()
    for _ in range(2):
        [o.zero_() for o in outs]
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, e) for o, e in zip(outs, eager))
    # a row does not depend on its neighbours in the block
    x[2, 77] = float("nan")
    sn, yn, _ = both()
    assert all(torch.equal(o[[0, 1, 3, 4]], e[[0, 1, 3, 4]])
               for o, e in zip((sn, yn), eager))
    assert yn[2].isnan().all() and sn[2].isnan().sum() == 1
    yg = torch.randn(3, 80, device="cuda").to(dtype)
    yg[1, 5], yg[2, 47] = float("nan"), float("nan")     # an a and a gate
    assert ops.geglu(yg).isnan().nonzero().tolist() == [[1, 5], [2, 7]]
    e = torch.empty(2, 0, 48, device="cuda", dtype=dtype)
    assert ops.layer_norm(e, w[:48], b[:48]).shape == e.shape
    assert ops.geglu(e).shape == (2, 0, 24) and ops.geglu(e[0].t()).shape == (48, 0)


def _launcher_refusals(dev="cuda"):
    x = torch.randn(4, 64, device=dev).to(C.BF16)
    w = torch.ones(64, device=dev, dtype=C.BF16)
    big = torch.ones(2, 2056, device=dev, dtype=C.BF16)
    return {"x on the CPU": (x.cpu(), w, w), "fp32 x": (x.float(), w, w),
            "fp16 weight": (x, w.half(), w), "bias on the CPU": (x, w, w.cpu()),
            "x unaligned": (x.flatten()[4:-4].view(-1, 8), w[:8], w[:8]),
            "C % 8": (x[:, :12].contiguous(), w[:12], w[:12]),
            "C > 2048": (big, big[0], big[0]),
            "x strided": (x[:, ::2], w[:32], w[:32]),
            "weight [C/2]": (x, w[:32], w), "delta shape": (x, w, w, x[:2]),
            "geglu N % 8": x[:, :24].contiguous(),
            "geglu strided": x.t().contiguous().t(),
            "geglu unaligned": x[:, 4:36]}


@pytest.mark.parametrize("what", list(_launcher_refusals("cpu")))
def test_launcher_refusal_leaves_the_next_call_right(what):
    args, ext = _launcher_refusals()[what], ops.hip_ext()
    x, _, w, b = (t.cuda() for t in ln_inputs("plain", 5, 320, C.BF16))
    want = ops.layer_norm(x, w, b)
    with pytest.raises(RuntimeError):
        if what.startswith("geglu"):
            ext.geglu(args)
        else:
            ext.layer_norm_affine(*args[:3], (args + (None,))[3], 1e-5)
    assert torch.equal(ops.layer_norm(x, w, b), want)


def test_fallbacks_warn_once_and_match_the_reference(caplog):
    ops._WARNED.clear()
    for x in (torch.randn(3, 64).cuda(),
              torch.randn(3, 2056).to(C.BF16).cuda()):
        w, b = torch.randn_like(x[:2])
        with caplog.at_level(logging.WARNING, logger="parallelanything.ops"):
            caplog.clear()
            for _ in range(2):
                s, y = ops.layer_norm(x, w, b, residual=x)
                out = ops.geglu(x[:, :24])
        assert len(caplog.records) == 2, caplog.text     # one per op, once
        assert all(torch.equal(o, r) for o, r in zip(
            (s, y), ops.reference.layer_norm(x, w, b, residual=x)))
        assert torch.equal(out, ops.reference.geglu(x[:, :24]))
