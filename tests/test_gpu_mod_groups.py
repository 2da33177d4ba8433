"""The grouped modulation kernels (ops/hip/mod_groups.h) against fp64, and
per-frame timesteps through the tiny WAN model on the device. x has mean 40
and group g a scale near g, a shift near 10 g and a gate near 1 + g, so a row
that takes its neighbour's group is off by hundreds of tolerances.
layer_norm_mod is held to kernel_cases.TOL_LN, gate_residual to the bits of
the rounded fp64 result, as the [B, D] kernels are."""
import copy

import pytest
import torch

import block_cases as C
import elementwise_cases as EW
import kernel_cases as K
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models.wan import WanConfig, WanDiT

pytestmark = pytest.mark.gpu

B = 2
DIMS = (8, 72, 520, 3072)       # one granule, partial slot, 2nd slot, a model
GROUPS = ((12, 1), (12, 3), (12, 12), (74, 2))  # 37 rows: runs 16 + 16 + 5
DTYPES = pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_IDS)
_CASES = {}


def case(S, G, D, dtype):
    """x, res, (scale, shift, gate) [3, B, G, D], the two fp64 results."""
    key = (S, G, D, dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(S * D + G)
        x = (40.0 + torch.randn(B, S, D, generator=g)).to(dtype)
        # res in eighths, the gate in 64ths, x in 32nds or coarser: gate * x
        # + res < 2^10 has 21 bits, so the kernel's fp32 sum rounds once
        res = (torch.randn(B, S, D, generator=g) * 8).round().div(8).to(dtype)
        idx = torch.arange(G, dtype=torch.float32)[None, :, None]
        mod = 0.1 * torch.randn(3, B, G, D, generator=g)
        mod[2] = (mod[2] * 64).round() / 64
        mod = (mod + torch.stack([idx, 10 * idx, 1 + idx])).to(dtype)
        _CASES[key] = (x, res, mod, *refs(x, res, mod))
    return _CASES[key]


def refs(x, res, mod):
    rows = torch.arange(x.shape[1]) // (x.shape[1] // mod.shape[2])
    scale, shift, gate = mod.double()[:, :, rows]
    return (K.layer_norm_f64(x) * (1.0 + scale) + shift,
            res.double() + gate * x.double())


def run(x, res, mod):
    scale, shift, gate = mod if mod[0].is_cuda else mod.cuda()
    return (ops.layer_norm_mod(x.cuda(), scale, shift),
            ops.gate_residual(res.cuda(), gate, x.cuda()))


@pytest.fixture(autouse=True)
def no_fallback(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "_unsupported", lambda *a: seen.append(a))
    yield
    assert not seen, f"ops fell back to the reference path: {seen}"


@DTYPES
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("S,G", GROUPS)
def test_against_fp64(S, G, D, dtype):
    x, res, mod, ln_ref, gate_ref = case(S, G, D, dtype)
    ln, gr = run(x, res, mod)
    K.check(ln, ln_ref, *K.TOL_LN, what="layer_norm_mod")
    EW.same_bits(gr.cpu(), gate_ref.to(dtype), "gate_residual")


def test_inputs_tell_the_groups_apart():
    x, res, mod, ln_ref, gate_ref = case(12, 3, 72, K.BF16)
    ln_swap, gate_swap = refs(x, res, mod[:, :, [1, 0, 2]])
    assert not K.passes(ln_swap.to(K.BF16), ln_ref, *K.TOL_LN)
    assert (ln_swap - ln_ref)[:, :8].abs().min() > 100 * K.TOL_LN[1]
    assert (gate_swap - gate_ref)[:, :8].abs().min() > 10.0


@DTYPES
@pytest.mark.parametrize("D", (72, 3072))
def test_indexing_twins(D, dtype):
    """[B, 1, D], its rows expanded to [B, G, D] and to [B, S, D], as
    stride-0 views and dense: one kernel, only the indexing differs."""
    x, res, mod, *_ = case(74, 1, D, dtype)
    want = run(x, res, mod)
    for G in (2, 74):
        wide = mod.cuda().expand(3, B, G, D)
        for got in (run(x, res, wide), run(x, res, wide.contiguous())):
            assert all(torch.equal(w, a) for w, a in zip(want, got)), G


@DTYPES
def test_strided_modulation(dtype):
    """The unbind(-2) views of a [B, G, 6, D] buffer whose other slots hold
    NaN, against contiguous clones."""
    x, res, mod, *_ = case(74, 2, 520, dtype)
    buf = torch.full((B, 2, 6, 520), float("nan"), dtype=dtype, device="cuda")
    buf[:, :, 1], buf[:, :, 3], buf[:, :, 4] = mod.cuda()
    views = buf.unbind(-2)
    assert not views[1].is_contiguous()
    got = run(x, res, (views[1], views[3], views[4]))
    assert all(torch.equal(w, a) for w, a in zip(run(x, res, mod), got))


def test_refusals_and_empties_are_followed_by_a_valid_call():
    x, res, mod, ln_ref, _ = case(12, 3, 72, K.BF16)
    xd, (scale, shift, gate) = x.cuda(), mod.cuda()
    bad = [(ValueError, scale[:, :1].expand(B, 5, 72)),
           (RuntimeError, scale[:1]), (RuntimeError, scale[..., :64]),
           (RuntimeError, scale.half()), (RuntimeError, scale.cpu())]
    for err, m in bad:
        with pytest.raises(err):
            ops.layer_norm_mod(xd, m, m)
        with pytest.raises(err):
            ops.gate_residual(xd, m, xd)
        K.check(ops.layer_norm_mod(xd, scale, shift), ln_ref, *K.TOL_LN)
    with pytest.raises(RuntimeError):
        ops.layer_norm_mod(xd, scale, shift[:, :1])
    for e, m in ((xd[:, :0], scale), (xd[:0], scale[:0]),
                 (xd[..., :0], scale[..., :0])):
        assert ops.layer_norm_mod(e, m, m).shape == e.shape
        assert ops.gate_residual(e, m, e).shape == e.shape
    K.check(ops.layer_norm_mod(xd, scale, shift), ln_ref, *K.TOL_LN)


@DTYPES
def test_tiny_wan_per_frame_timesteps(dtype):
    """Against the fp32 CPU model, within the suite's whole-model bound:
    M_MODEL x the CPU ``dtype`` forward's distance from that reference."""
    torch.manual_seed(0)
    master = WanDiT(WanConfig.tiny()).eval().to(dtype).float()
    x = torch.randn(2, 4, 3, 8, 12).to(dtype)   # f = 3 frames of 4 x 6 tokens
    ctx = torch.randn(2, 5, 32).to(dtype)
    t = torch.tensor([[0.0, 0.5, 0.9], [0.0, 0.2, 0.7]])

    def forward(device, dt):
        model = copy.deepcopy(master).to(device=device, dtype=dt)
        return model(x.to(device, dt), t.to(device),
                     context=ctx.to(device, dt))
    ref = forward("cpu", torch.float32)
    e_ref = C.rel_l2(forward("cpu", dtype), ref)
    e_gpu = C.rel_l2(forward("cuda", dtype), ref)
    print(f"\ntiny wan [B, f] {dtype}: {e_gpu:.3e} / {e_ref:.3e}")
    assert e_gpu <= C.M_MODEL[dtype] * e_ref
