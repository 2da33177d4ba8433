"""The rotary, packing, gating and timestep kernels on the cases of
elementwise_cases.py: qk_norm_rope_, pack_joint_qkv, rope_apply,
gate_residual, gelu_tanh's large launches, timestep_embedding and
timestep_embed_mlp (test_elementwise_cases_reference.py shows on the CPU
that these checks reject a subtly wrong kernel).

16-bit outputs are held to 0.5 + SLACK spacings of their own type against
fp64, the exact cases to bit equality, everything outside a view to its
bits before the call, and the timestep sinusoid to TS_A + TS_B |arg| 2^-24
up to |arg| = 14610 and beyond.
"""
import pytest
import torch

import elementwise_cases as E
from comfyui_parallelanything_amd import ops

pytestmark = pytest.mark.gpu

NATIVE = ("qk_norm_rope_", "pack_joint_qkv", "rope_apply", "gate_residual",
          "gelu_tanh", "timestep_embedding", "timestep_embed_mlp")


@pytest.fixture(scope="module")
def device():
    for op in NATIVE:
        assert ops.hip_available(op)
    return E.OpsBackend("cuda")


@pytest.mark.parametrize("name", sorted(E.CHECKS))
def test_elementwise(name, device):
    E.CHECKS[name](device)


# ---- refusals: raised before any launch, and the next valid call is right --

@pytest.mark.parametrize("name", sorted(E.REFUSALS))
def test_refused(name, device):
    with pytest.raises(RuntimeError):
        E.REFUSALS[name](ops, "cuda")
    torch.cuda.synchronize()
    E.CHECKS[E.after_refusal(name)](device)


@pytest.mark.parametrize("op,i", [(op, i)
                                  for op, (_, idx) in
                                  sorted(E.DEVICE_REFUSALS.items())
                                  for i in idx])
def test_refused_argument_on_the_cpu(op, i, device):
    with pytest.raises(RuntimeError):
        E.DEVICE_REFUSALS[op][0](ops, "cuda", i)
    torch.cuda.synchronize()
    E.CHECKS[E.after_refusal(op)](device)


def test_gate_residual_refuses_cpu_gate(device):
    x = torch.zeros(2, 3, 8, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.gate_residual(x, torch.zeros(2, 8, dtype=torch.bfloat16), x)
    with pytest.raises(RuntimeError):
        ops.gate_residual(x.cpu(), x[:, 0].contiguous(), x)
    torch.cuda.synchronize()
    E.CHECKS["gate vec bf16"](device)


# ---- empties: the right shape, no launch, nothing left pending -------------

@pytest.mark.parametrize("name", sorted(E.EMPTIES))
def test_empty(name, device):
    E.EMPTIES[name](ops, "cuda")
    torch.cuda.synchronize()
    E.CHECKS["gate scalar bf16"](device)


def test_timestep_embed_mlp_empty_batch(device):
    w1 = torch.zeros(16, 8, device="cuda", dtype=torch.bfloat16)
    out = ops.timestep_embed_mlp(torch.zeros(0, device="cuda"), w1, None)
    assert out.shape == (0, 16)
    torch.cuda.synchronize()


def test_timestep_embedding_dim_1_is_the_zero_column(device):
    t = torch.tensor([0.5, 4.0], device="cuda")
    out = ops.timestep_embedding(t, 1)
    assert out.shape == (2, 1) and out.dtype == torch.float32
    assert (out == 0).all()
