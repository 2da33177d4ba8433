"""The fp8 (e4m3fn) emit kernels bit for bit: quant_fp8, gelu_fp8,
layer_norm_mod_fp8 and the delayed-scaling finalize, through the checks of
fp8_cases.py (test_fp8_cases_reference.py shows on the CPU that those checks
reject a subtly wrong kernel).

quant_fp8's output bytes and the whole state (scale, amax_buf, scale_used)
must equal the plain-torch reference; the fused ops, whose fp32 values
differ from fp64 ones, are held to the off-tie criterion and to their state.
"""
import pytest
import torch

import fp8_cases as F8
from comfyui_parallelanything_amd import ops

pytestmark = pytest.mark.gpu


class Device:
    """The backend of fp8_cases.CHECKS that runs the native kernels: CPU
    tensors in, CPU bytes out, the state read back into `st`."""

    @staticmethod
    def _state(st):
        scale, amax = st.scale.cuda(), st.amax.cuda()
        used = scale if st.aliased else st.used.cuda()
        return scale, amax, used

    @staticmethod
    def _read(st, scale, amax, used):
        st.scale.copy_(scale.cpu())
        st.amax.copy_(amax.cpu())
        if not st.aliased:
            st.used.copy_(used.cpu())

    def _run(self, fn, st):
        scale, amax, used = self._state(st)
        out = fn(scale, amax, used)
        assert out.dtype == torch.float8_e4m3fn
        self._read(st, scale, amax, used)
        return out.view(torch.uint8)

    def quant(self, x, st):
        xd = x.cuda()
        if st.aliased:      # the public default: no scale_used buffer
            return self._run(lambda s, a, u: ops.quant_fp8(xd, s, a), st).cpu()
        return self._run(
            lambda s, a, u: ops.quant_fp8(xd, s, a, scale_used=u), st).cpu()

    def gelu(self, x, st):
        xd = x.cuda()
        return self._run(lambda s, a, u: ops.gelu_fp8(xd, s, a, u), st).cpu()

    def ln(self, x, sc, sh, st):
        xd, scd, shd = x.cuda(), sc.cuda(), sh.cuda()
        return self._run(lambda s, a, u: ops.layer_norm_mod_fp8(
            xd, scd, shd, s, a, u, F8.LN_EPS), st).cpu().flatten()

    def large(self, op, pattern, nvec, st):
        """The input is tiled on the device and the bytes stay there: the
        check compares them with the tiled reference where they are."""
        idx = torch.arange(nvec, device="cuda") % F8.PERIOD
        xd = pattern.cuda()[idx].reshape(-1)
        del idx
        fn = ops.quant_fp8 if op == "quant" else ops.gelu_fp8
        return self._run(lambda s, a, u: fn(xd, s, a, u), st).view(nvec, 8)


@pytest.mark.parametrize("name", sorted(F8.CHECKS))
def test_fp8_emit(name):
    for op in ("quant_fp8", "gelu_fp8", "layer_norm_mod_fp8"):
        assert ops.hip_available(op)
    F8.CHECKS[name](Device())


# ---- layer_norm_mod_fp8 refuses a modulation it would misread -------------

def _ln_args(B=2, S=3, D=64):
    x = torch.randn(B, S, D, device="cuda", dtype=torch.bfloat16)
    sc = torch.zeros(B, D, device="cuda", dtype=torch.bfloat16)
    sh = torch.zeros(B, D, device="cuda", dtype=torch.bfloat16)
    return x, sc, sh


def _refused(x, sc, sh):
    """Raises, and before any launch: the state is untouched."""
    qscale = torch.full((1,), 0.25, device="cuda")
    amax = torch.tensor([3.0, 0.0], device="cuda")
    used = torch.zeros(1, device="cuda")
    with pytest.raises(RuntimeError):
        ops.layer_norm_mod_fp8(x, sc, sh, qscale, amax, used)
    torch.cuda.synchronize()
    assert qscale.item() == 0.25 and used.item() == 0.0
    assert amax.tolist() == [3.0, 0.0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16],
                         ids=["fp32", "fp16"])
@pytest.mark.parametrize("which", ["scale", "shift"])
def test_layer_norm_mod_fp8_refuses_modulation_dtype(which, dtype):
    x, sc, sh = _ln_args()
    if which == "scale":
        _refused(x, sc.to(dtype), sh)
    else:
        _refused(x, sc, sh.to(dtype))


@pytest.mark.parametrize("which", ["scale", "shift"])
def test_layer_norm_mod_fp8_refuses_cpu_modulation(which):
    x, sc, sh = _ln_args()
    if which == "scale":
        _refused(x, sc.cpu(), sh)
    else:
        _refused(x, sc, sh.cpu())


@pytest.mark.parametrize("shape", [(2, 3, 64), (2, 56), (2, 72), (1, 64),
                                   (3, 64), (128,)],
                         ids=lambda s: "x".join(map(str, s)))
def test_layer_norm_mod_fp8_refuses_modulation_shape(shape):
    """[B, S, D], a wrong D, a wrong B and a flat tensor, for x [2, 3, 64]."""
    x, sc, sh = _ln_args()
    bad = torch.zeros(shape, device="cuda", dtype=torch.bfloat16)
    _refused(x, bad, bad.clone())
    _refused(x, bad, sh)
    _refused(x, sc, bad)
