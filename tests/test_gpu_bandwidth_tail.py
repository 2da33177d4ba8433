"""The memory-bound tail of the MMDiT step, bit for bit.

qk_norm_rope_ and pack_joint_qkv take a token-major kernel when D is 128 or
64, the heads of a token are contiguous and every base and stride is a
multiple of 16 bytes, and the generic kernel otherwise; the two must give
the same bits. layer_norm_mod and gate_residual read scale, shift and gate
at their row stride (column slices of the banked modulation GEMM) and copy
only what they cannot read; a slice and its contiguous copy must give the
same bits, and so must a block fed either.

Every comparison is torch.equal on seeded inputs of mixed scale with one row
scaled by 30 and one all-zero row. Accuracy against fp64 is held by
test_gpu_elementwise_exact.py, test_gpu_norm_regimes.py and
test_gpu_blocks.py on the same entry points.
"""
import pytest
import torch

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models import layers as L

pytestmark = pytest.mark.gpu

DTYPES16 = [torch.bfloat16, torch.float16]
IDS16 = ["bf16", "fp16"]
GUARD = 64          # elements each side of a view; 128 bytes keeps alignment
SENTINEL = 777.0


@pytest.fixture(scope="module", autouse=True)
def require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for op in ("qk_norm_rope_", "pack_joint_qkv", "layer_norm_mod",
               "gate_residual"):
        assert ops.hip_available(op)


def _values(shape, seed, dtype):
    """Uniform [-1, 1) times 2^[-3, 3] per row of the last dim, the first
    row scaled by 30 and the last one zero; rounded to dtype, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g) * 2 - 1
    e = torch.randint(-3, 4, shape[:-1] + (1,), generator=g)
    v = v * torch.pow(2.0, e.float())
    flat = v.view(-1, shape[-1])
    flat[0] *= 30
    flat[-1] = 0
    return v.to(dtype)


def _cs(S, D, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(S, D // 2, generator=g) * 6.2831853
    return torch.stack([a.cos(), a.sin()], dim=-1).cuda()


def _weights(n, D, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(D, generator=g) + 0.5).to(dtype).cuda()
            for _ in range(n)]


class Layout:
    """vals ([..., 3, H, D]) placed in a buffer on the GPU.

    'dense': the [..., 3, H, D] buffer itself, 16-byte aligned (the token-
    major kernels). 'offset': the same, based 2 elements in. 'padded':
    [..., :D] of a [..., 3, H, D + 2] buffer. Either of the last two takes
    the generic kernels. Guard elements and pad columns hold SENTINEL."""

    def __init__(self, vals, kind):
        self.kind = kind
        D = vals.shape[-1]
        shape = list(vals.shape)
        if kind == "padded":
            shape[-1] = D + 2
        n = 1
        for s in shape:
            n *= s
        lead = GUARD + (2 if kind == "offset" else 0)
        self.flat = torch.full((lead + n + GUARD,), SENTINEL,
                               dtype=vals.dtype, device="cuda")
        self.full = self.flat[lead:lead + n].view(shape)
        self.view = self.full[..., :D]
        self.view.copy_(vals)
        self.lead, self.n = lead, n
        self.before = self.flat.clone()

    def outside_unchanged(self):
        ok = torch.equal(self.flat[:self.lead], self.before[:self.lead])
        ok &= torch.equal(self.flat[self.lead + self.n:],
                          self.before[self.lead + self.n:])
        if self.kind == "padded":
            D = self.view.shape[-1]
            ok &= bool((self.full[..., D:] == SENTINEL).all())
        return ok

    def unchanged(self):
        return torch.equal(self.flat, self.before)


def _other_layouts(H):
    # with one head there is no head stride to pad
    return ["offset"] if H == 1 else ["offset", "padded"]


QK_SHAPES = [(2, 5, 3), (1, 1, 1), (2, 70, 24)]


def _qk_cases():
    for B, S, H in QK_SHAPES:
        for D in (128, 64):
            for dt, name in zip(DTYPES16, IDS16):
                if (B, S, H) == (2, 70, 24) and (D, name) != (128, "bf16"):
                    continue        # one case of several blocks
                yield pytest.param(B, S, H, D, dt,
                                   id=f"B{B}S{S}H{H}D{D}-{name}")


@pytest.mark.parametrize("B,S,H,D,dtype", list(_qk_cases()))
def test_qk_norm_rope_token_major_equals_generic(B, S, H, D, dtype):
    vals = _values((B, S, 3, H, D), 11, dtype)
    wq, wk = _weights(2, D, 12, dtype)
    cs = _cs(S, D, 13)
    results = {}
    for kind in ["dense"] + _other_layouts(H):
        lay = Layout(vals, kind)
        q, k, v = lay.view.unbind(2)
        ops.qk_norm_rope_(q, k, wq, wk, cs)
        torch.cuda.synchronize()
        assert lay.outside_unchanged(), kind
        assert torch.equal(v.cpu(), vals[:, :, 2]), kind
        results[kind] = (q.cpu(), k.cpu())
    rq, rk = results.pop("dense")
    assert not torch.equal(rq, vals[:, :, 0]) or B * S * H == 0
    for kind, (gq, gk) in results.items():
        assert torch.equal(rq, gq), f"q: dense vs {kind}"
        assert torch.equal(rk, gk), f"k: dense vs {kind}"


PACK_SHAPES = [(2, 3, 5, 3), (2, 0, 5, 3), (2, 64, 70, 24)]


def _pack_cases():
    for B, T, Si, H in PACK_SHAPES:
        for D in (128, 64):
            for dt, name in zip(DTYPES16, IDS16):
                if (T, Si, H) == (64, 70, 24) and (D, name) != (128, "bf16"):
                    continue
                yield pytest.param(B, T, Si, H, D, dt,
                                   id=f"B{B}T{T}Si{Si}H{H}D{D}-{name}")


@pytest.mark.parametrize("B,T,Si,H,D,dtype", list(_pack_cases()))
def test_pack_joint_qkv_token_major_equals_generic(B, T, Si, H, D, dtype):
    tv = _values((B, max(T, 1), 3, H, D), 21, dtype)[:, :T]
    iv = _values((B, Si, 3, H, D), 22, dtype)
    w = _weights(4, D, 23, dtype)
    cs = _cs(T + Si, D, 24)
    results = {}
    # both streams in one layout, then one stream eligible and the other not
    kinds = [(k, k) for k in ["dense"] + _other_layouts(H)]
    kinds += [("dense", "offset"), ("offset", "dense")]
    if H > 1:
        kinds.append(("dense", "padded"))
    for kind in kinds:
        lt, li = Layout(tv.contiguous(), kind[0]), Layout(iv, kind[1])
        q, k, v = ops.pack_joint_qkv(lt.view, li.view, *w, cs)
        torch.cuda.synchronize()
        assert lt.unchanged() and li.unchanged(), kind
        assert all(t.is_contiguous() and t.shape == (B, T + Si, H, D)
                   for t in (q, k, v))
        assert torch.equal(v.cpu(), torch.cat([tv[:, :, 2], iv[:, :, 2]], 1))
        results[kind] = (q.cpu(), k.cpu())
    rq, rk = results.pop(("dense", "dense"))
    for kind, (gq, gk) in results.items():
        assert torch.equal(rq, gq), f"q: dense vs {kind}"
        assert torch.equal(rk, gk), f"k: dense vs {kind}"


# ---- row-strided modulation operands ----------------------------------------

def _bank(B, D, dtype, start=0, extra=0):
    """Five [B, D] column slices of one [B, 5 D + start + extra] tensor
    with distinct rows and a guard after the last row."""
    width = 5 * D + start + extra
    flat = torch.full((B * width + GUARD,), SENTINEL, dtype=dtype,
                      device="cuda")
    bank = flat[:B * width].view(B, width)
    bank.copy_(_values((B, width), 31, dtype) * 0.25)
    slices = [bank[:, start + i * D:start + (i + 1) * D] for i in range(5)]
    return flat, slices


MOD_LAYOUTS = {
    "aligned": dict(start=0, extra=0),      # read in place by the vec kernels
    "8-byte base": dict(start=4, extra=4),  # copied for the vec kernels
    "odd stride": dict(start=0, extra=4),   # row stride % 8 != 0: copied
}


@pytest.mark.parametrize("layout", sorted(MOD_LAYOUTS))
@pytest.mark.parametrize("D", [3072, 72, 20])
@pytest.mark.parametrize("dtype", DTYPES16 + [torch.float32],
                         ids=IDS16 + ["fp32"])
def test_strided_modulation_equals_contiguous(dtype, D, layout):
    B, S = 2, 3
    flat, (scale, _, shift, gate, _) = _bank(B, D, dtype, **MOD_LAYOUTS[layout])
    assert not scale.is_contiguous()
    before = flat.clone()
    x = _values((B, S, D), 32, dtype).cuda()
    res = _values((B, S, D), 33, dtype).cuda()

    got = ops.layer_norm_mod(x, scale, shift)
    want = ops.layer_norm_mod(x, scale.contiguous(), shift.contiguous())
    assert torch.equal(got, want)
    # rows are distinct: the wrong row of scale or shift shows
    swapped = ops.layer_norm_mod(x, scale.flip(0).contiguous(),
                                 shift.flip(0).contiguous())
    assert not torch.equal(got, swapped)

    got = ops.gate_residual(res, gate, x)
    want = ops.gate_residual(res, gate.contiguous(), x)
    assert torch.equal(got, want)
    assert not torch.equal(got, ops.gate_residual(
        res, gate.flip(0).contiguous(), x))
    torch.cuda.synchronize()
    assert torch.equal(flat, before)


def test_strided_modulation_refusals_stay():
    x = torch.zeros(2, 3, 16, device="cuda", dtype=torch.bfloat16)
    bank = torch.zeros(2, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):      # broadcast gate
        ops.gate_residual(x, bank[:1, :16], x)
    with pytest.raises(RuntimeError):      # another D
        ops.gate_residual(x, bank[:, :24], x)
    with pytest.raises(RuntimeError):      # another dtype
        ops.layer_norm_mod(x, bank[:, :16].float(), bank[:, 16:32].float())
    with pytest.raises(RuntimeError):      # another D
        ops.layer_norm_mod(x, bank[:, :24], bank[:, 24:48])
    torch.cuda.synchronize()


# ---- blocks fed banked (strided) and contiguous modulations -----------------

def _dense(mod):
    return None if mod is None else L.ModOut(
        mod.shift.contiguous(), mod.scale.contiguous(), mod.gate.contiguous())


@pytest.mark.parametrize("dtype", DTYPES16, ids=IDS16)
def test_blocks_with_banked_modulations(dtype):
    torch.manual_seed(41)
    hidden, heads, B, T, side = 128, 2, 2, 8, 4
    double = L.DoubleStreamBlock(hidden, heads).to("cuda", dtype).eval()
    single = L.SingleStreamBlock(hidden, heads).to("cuda", dtype).eval()
    bank = L.ModulationBank([double.img_mod, double.txt_mod,
                             single.modulation])
    img = _values((B, side * side, hidden), 42, dtype).cuda()
    txt = _values((B, T, hidden), 43, dtype).cuda()
    vec = _values((B, hidden), 44, dtype).cuda()
    pe = L.rope_2d_table(side, side, (16, 24, 24), device="cuda", text_len=T)
    with torch.no_grad():
        m_img, m_txt, m_single = bank(vec)
        assert not m_img[0].scale.is_contiguous()
        outs = []
        for dense in (False, True):
            f = (lambda m: tuple(_dense(p) for p in m)) if dense else (
                lambda m: m)
            i2, t2 = double(img, txt, vec, pe, mods=(f(m_img), f(m_txt)))
            x = torch.cat([t2, i2], dim=1)
            outs.append((i2, t2, single(x, vec, pe,
                                        mods=(f(m_single)[0],))))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b)
