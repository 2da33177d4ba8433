"""ops.layer_norm / ops.geglu and the UNet token_ops mode. On the CPU the
ops are the torch composition the block runs by default; the cases marked
gpu run on the native path (the kernels: test_gpu_token_ops.py)."""
import pytest
import torch
import torch.nn.functional as F

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models import sd_unet as U
from comfyui_parallelanything_amd.models.registry import MODELS


@pytest.mark.parametrize("dtype",
                         (torch.float32, torch.bfloat16, torch.float16))
def test_cpu_ops_are_the_torch_composition(dtype):
    x, delta = torch.randn(2, 5, 40).to(dtype)
    w, b = torch.randn(2, 40).to(dtype)
    assert torch.equal(ops.layer_norm(x, w, b),
                       F.layer_norm(x, (40,), w, b, 1e-5))
    s, ys = ops.layer_norm(delta, w, b, 1e-6, residual=x)
    assert torch.equal(s, x + delta)
    assert torch.equal(ys, F.layer_norm(s, (40,), w, b, 1e-6))
    assert torch.equal(ops.geglu(x), x[:, :20] * F.gelu(x[:, 20:]))
    assert ops.layer_norm(x[:0], w, b).shape == (0, 40)
    assert ops.geglu(x[:0]).shape == (0, 20) and ops.geglu(x[:, :0]).shape == (5, 0)


@pytest.mark.parametrize("dev, dtype", [
    ("cpu", torch.float32),
    pytest.param("cuda", torch.bfloat16, marks=pytest.mark.gpu)])
def test_what_no_path_accepts_raises(dev, dtype):
    x = torch.randn(3, 16, device=dev).to(dtype)
    w = torch.ones(16, device=dev, dtype=dtype)
    for args, kw in (((x, torch.cat([w, w[:8]]), w), {}),     # weight [C + 8]
                     ((x, w, w[None]), {}),                   # bias 2-D
                     ((x, w.double(), w), {}),                # weight dtype
                     ((x, w, w.to("meta")), {}),              # bias device
                     ((x, w, w), {"residual": x[:2]}),
                     ((x, w, w), {"residual": x.double()})):
        with pytest.raises(RuntimeError, match="layer_norm"):
            ops.layer_norm(*args, **kw)
    for y in (x[:, :15], x[0, 0]):                  # odd last dim, 0-d
        with pytest.raises(RuntimeError, match="geglu"):
            ops.geglu(y)


@pytest.mark.parametrize("name", ["sd15", "sdxl"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dev, dtype", [("cpu", torch.float32)] + [
    pytest.param("cuda", d, marks=pytest.mark.gpu)
    for d in (torch.bfloat16, torch.float16)])
def test_token_ops_model(dev, dtype, channels_last, name, monkeypatch):
    """CPU, fp32: bitwise the default model. GPU, 16 bits: from the fp64
    forward, token_ops may be max(1, 4 k) = 4 times as far as the default is
    (its own distance as the unit: test_channels_last_forward_matches_default)."""
    make, inputs = MODELS[name]
    kw_m = dict(dev=dev, dtype=dtype, tiny=True, channels_last=channels_last)
    m, mt = make(**kw_m), make(token_ops=True, **kw_m)
    assert mt.cfg.token_ops and not m.cfg.token_ops and \
        list(m.state_dict()) == list(mt.state_dict())
    torch.manual_seed(5)
    m.load_state_dict({k: (torch.randn_like(v.float()) * 0.05).to(dtype)
                       for k, v in m.state_dict().items()})
    mt.load_state_dict(m.state_dict())
    x, t, c, kw = inputs(2, tiny=True, dev=dev, dtype=dtype, text_len=[3, 8])
    # [layer_norm, geglu] calls of every TransformerBlock, and no fallback
    seen, fell = [], []
    monkeypatch.setattr(ops, "_unsupported", lambda *a: fell.append(a))
    out_def = m(x, t, context=c, **kw)
    for i, op in enumerate(("layer_norm", "geglu")):
        def counted(*a, _fn=getattr(ops, op), _i=i, **k):
            seen[-1][_i] += 1
            return _fn(*a, **k)
        monkeypatch.setattr(ops, op, counted)
    for mod in mt.modules():
        if isinstance(mod, U.TransformerBlock):
            mod.register_forward_pre_hook(lambda *_: seen.append([0, 0]))
    out = mt(x, t, context=c, **kw)
    assert seen and all(s == [3, 1] for s in seen) and not fell, (seen, fell)
    if dev == "cpu":
        assert torch.equal(out, out_def)
        m.use_token_ops().load_state_dict(mt.state_dict())  # the other way
        assert torch.equal(m(x, t, context=c, **kw), out)
        monkeypatch.setenv("PA_UNET_TOKEN_OPS", "1")
        assert make(tiny=True, dtype=dtype).cfg.token_ops
        return
    wide = lambda v: v.cpu().double() if v.is_floating_point() else v.cpu()
    ref = m.cpu().double()(wide(x), wide(t), context=wide(c),
                           **{k: wide(v) for k, v in kw.items()})
    e_def, e_tok = ((o.double().cpu() - ref).abs().max().item()
                    for o in (out_def, out))
    print(f"{name}: from fp64, default {e_def:.3e}, token_ops {e_tok:.3e}, "
          f"ratio {e_tok / e_def:.3f}")
    assert e_tok <= 4.0 * e_def
