"""ops.group_norm and the channels-last UNet mode, on the CPU.

The op against fp64 on the rows of kernel_cases.py (the GPU file runs the
same comparison on the native kernels), the identities of the reference
path, its refusals, and the channels-last tiny models against the default
ones.
"""
import copy

import pytest
import torch

import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models import sd_unet as U
from comfyui_parallelanything_amd.models.registry import MODELS
from comfyui_parallelanything_amd.ops import reference as R

from group_norm_cases import (CL, check_rows, group_norm_f64, is_cl,
                              refusals, run_regimes)

F32 = torch.float32


def _op(x, G, w, b, eps, silu, add):
    return ops.group_norm(x, G, w, b, eps, silu=silu, channel_add=add)


@pytest.mark.parametrize("shape", C.GN_SHAPES, ids=["n18", "n280", "cpg1"])
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
def test_group_norm_against_fp64(dtype, shape):
    run_regimes(shape, dtype, _op)


# ---------------- reference identities ----------------

def test_channel_add_is_the_unrounded_sum():
    x = C.offset(2, 32 * 5 * 7, C.BF16, 3).reshape(2, 32, 5, 7)
    add = C.plain(2, 32, C.BF16, 4)
    w, b = C.plain(1, 32, C.BF16, 7)[0], C.plain(1, 32, C.BF16, 8)[0]
    for silu in (False, True):
        got = R.group_norm(x, 4, w, b, silu=silu, channel_add=add)
        want = R.group_norm(x.float() + add.float()[:, :, None, None], 4,
                            w.float(), b.float(), silu=silu).to(C.BF16)
        assert torch.equal(got, want)
        # the rounded sum is something else
        rounded = R.group_norm(x + add[:, :, None, None], 4, w, b, silu=silu)
        assert not torch.equal(got, rounded)


def test_memory_format_is_preserved():
    x = torch.randn(2, 16, 5, 3)
    y = ops.group_norm(x, 4)
    assert y.is_contiguous() and not is_cl(y)
    yc = ops.group_norm(x.contiguous(memory_format=CL), 4)
    assert is_cl(yc) and not yc.is_contiguous()
    assert torch.equal(y, yc)
    assert yc.dtype == x.dtype and yc.shape == x.shape


def test_tokens_are_a_view_of_a_channels_last_result():
    B, Cn, H, W = 2, 16, 5, 3
    y = ops.group_norm(torch.randn(B, Cn, H, W).contiguous(memory_format=CL),
                       4)
    tok = y.permute(0, 2, 3, 1).reshape(B, H * W, Cn)
    assert tok.data_ptr() == y.data_ptr() and tok.is_contiguous()


def test_matches_group_norm_silu_and_nn_group_norm():
    x = torch.randn(2, 16, 4, 4)
    w, b = torch.randn(16), torch.randn(16)
    assert torch.equal(ops.group_norm(x, 4, w, b, silu=True),
                       ops.group_norm_silu(x, 4, w, b))
    gn = torch.nn.GroupNorm(4, 16, eps=1e-6)
    with torch.no_grad():
        gn.weight.copy_(w)
        gn.bias.copy_(b)
        assert torch.equal(ops.group_norm(x, 4, w, b), gn(x))


def test_empty_input():
    for shape in ((0, 16, 4, 4), (2, 16, 0, 4), (2, 16, 4, 0)):
        x = torch.empty(shape).contiguous(memory_format=CL)
        assert ops.group_norm(x, 4, silu=True).shape == x.shape


# ---------------- refusals ----------------

def test_refusals_raise_on_the_cpu():
    for what, args, kw in refusals():
        with pytest.raises(RuntimeError, match="group_norm"):
            ops.group_norm(*args, **kw)
        with pytest.raises(RuntimeError, match="group_norm"):
            R.group_norm(*args, **kw)


def test_other_device_is_refused():
    x = torch.randn(1, 8, 2, 2)
    meta = torch.ones(8, device="meta")
    with pytest.raises(RuntimeError, match="is on"):
        ops.group_norm(x, 4, meta, torch.ones(8))
    with pytest.raises(RuntimeError, match="is on"):
        ops.group_norm(x, 4, channel_add=torch.ones(1, 8, device="meta"))


# ---------------- models ----------------

# test_sequence_parallel.py's bound for "the same fp32 forward, summed in
# another order" is rtol=1e-5, atol=1e-6. It fits where the forward itself
# is well inside it from fp64, and the default tiny forwards are not: in
# units of that bound they are 0.76 and 0.90 (sd15, dense and masked), 0.69
# and 0.76 (sdxl) from their own fp64 run (largest difference 1.0e-6 to
# 1.2e-6 on outputs up to 1.4). So the bound is taken from that distance,
# by the rule kernel_cases uses for a reference (within a quarter of the
# tolerance): with k the default forward's distance from fp64 in units of
# (1e-5, 1e-6), both are scaled by max(1, 4 k), which is 2.8 to 3.6 here.
# For scale: the channels-last forwards measured 1.03 to 1.50 units from
# the default ones, and 1.9e-6 to 2.5e-6 from fp64 where the default is
# 1.2e-6; a default model given only channels-last conv weights and input
# is 2.2e-6 from fp64, so the difference is the library's NHWC convolution
# on the CPU.
RTOL, ATOL = 1e-5, 1e-6


def _wide(v):
    return v.double() if isinstance(v, torch.Tensor) and \
        v.is_floating_point() else v


def model_tol(m, ref, x, t, c, kw):
    """(rtol, atol) for a forward that should equal ``ref`` = m(...) up to
    fp32 summation order, from ref's own distance to the fp64 forward."""
    r64 = copy.deepcopy(m).double()(
        _wide(x), _wide(t), context=_wide(c),
        **{k: _wide(v) for k, v in kw.items()})
    k = ((ref.double() - r64).abs() / (ATOL + RTOL * r64.abs())).max().item()
    print(f"default forward is {k:.2f} x (1e-5, 1e-6) from fp64")
    assert k < 2.0, f"the default fp32 forward is {k:.2f} units from fp64"
    scale = max(1.0, 4.0 * k)
    return dict(rtol=RTOL * scale, atol=ATOL * scale)


FAMILIES = pytest.mark.parametrize("name", ["sd15", "sdxl"])


def _pair(name):
    make, inputs = MODELS[name]
    m = make(tiny=True, dtype=F32)
    mc = make(tiny=True, dtype=F32, channels_last=True)
    assert mc.cfg.channels_last and not m.cfg.channels_last
    return m, mc, inputs


@FAMILIES
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "keymask"])
def test_channels_last_forward_matches_default(name, masked):
    m, mc, inputs = _pair(name)
    x, t, c, kw = inputs(2, tiny=True, dtype=F32,
                         text_len=[3, 8] if masked else None)
    ref = m(x, t, context=c, **kw)
    out = mc(x, t, context=c, **kw)
    assert out.shape == ref.shape and out.shape[1] == 4
    assert out.is_contiguous() and out.stride() == ref.stride()
    torch.testing.assert_close(out, ref, **model_tol(m, ref, x, t, c, kw))


@FAMILIES
def test_state_dicts_are_interchangeable(name):
    m, mc, inputs = _pair(name)
    assert list(m.state_dict()) == list(mc.state_dict())
    assert [n for n, _ in m.named_modules()] == \
        [n for n, _ in mc.named_modules()]
    x, t, c, kw = inputs(2, tiny=True, dtype=F32)
    torch.manual_seed(5)
    sd = {k: torch.randn_like(v) * 0.05 for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    ref = m(x, t, context=c, **kw)
    # default -> channels-last
    mc.load_state_dict(m.state_dict())
    out = mc(x, t, context=c, **kw)
    torch.testing.assert_close(out, ref, **model_tol(m, ref, x, t, c, kw))
    assert all(is_cl(p.weight) for p in mc.modules()
               if isinstance(p, torch.nn.Conv2d)), "weights left NHWC"
    # channels-last -> default
    m2 = MODELS[name][0](tiny=True, dtype=F32)
    m2.load_state_dict(mc.state_dict())
    assert torch.equal(m2(x, t, context=c, **kw), ref)


@FAMILIES
def test_to_channels_last_on_a_built_model(name):
    m, mc, inputs = _pair(name)
    x, t, c, kw = inputs(2, tiny=True, dtype=F32)
    m2 = copy.deepcopy(m).to_channels_last()
    assert torch.equal(m2(x, t, context=c, **kw), mc(x, t, context=c, **kw))


def test_env_switch(monkeypatch):
    monkeypatch.setenv("PA_CHANNELS_LAST", "1")
    assert MODELS["sdxl"][0](tiny=True, dtype=F32).cfg.channels_last
    monkeypatch.setenv("PA_CHANNELS_LAST", "0")
    assert not MODELS["sd15"][0](tiny=True, dtype=F32).cfg.channels_last


@FAMILIES
def test_layout_survives_the_whole_forward(name):
    """torch.cat of the skips, nearest upsampling, the strided downsample
    conv, the 1x1 skip convs and the transformer's way back all keep
    channels-last: every GNSiLU and SpatialTransformer sees it."""
    _, mc, inputs = _pair(name)
    seen = []

    def hook(mod, args):
        seen.append((type(mod).__name__, args[0].shape[1], is_cl(args[0])))

    kinds = (U.GNSiLU, U.SpatialTransformer)
    n = 0
    for mod in mc.modules():
        if isinstance(mod, kinds):
            mod.register_forward_pre_hook(hook)
            n += 1
    x, t, c, kw = inputs(2, tiny=True, dtype=F32)
    mc(x, t, context=c, **kw)
    assert len(seen) == n and n > 10
    assert all(ok for _, _, ok in seen), [s for s in seen if not s[2]]


def test_cli_flag(capsys):
    from comfyui_parallelanything_amd.cli import main

    main(["--model", "sd15", "--devices", "cpu,cpu", "--batch", "2",
          "--steps", "1", "--tiny", "--channels-last"])
    with pytest.raises(SystemExit):
        main(["--model", "flux", "--tiny", "--channels-last"])
