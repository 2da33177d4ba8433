"""Cases, taps and fp64 references for the model blocks (models/layers.py,
models/wan.py, models/sd_unet.py): the layer that picks the strided views,
rotary rows, norm weights, masks and split points the kernels receive.

A block's output cannot carry a wiring test: the residual swamps the branch,
and a rotary table shifted by one row moves the output by about as much as
bf16 rounding does. So every ``ops.*`` call of one forward is a tap
(Recorder), each tap is compared with the same block in fp64, and the
yardstick at a tap is the distance of the CPU 16-bit reference path from
fp64 at that tap:

    e(tap)  = |tap - tap_fp64| / |tap_fp64|                 (rel-l2)
    limit   = M[dtype] * e_ref(tap),  e_ref from the CPU run of that dtype

tests/test_block_cases_reference.py shows on the CPU that the two fp64
references below agree to 1e-9 and that every fault in FAULTS moves a named
tap by at least twice the limit; tests/test_gpu_blocks.py holds the native
path to the limit. docs/KERNELS.md, "Block composition".
"""
from __future__ import annotations

import contextlib
import copy
import math
import zlib
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch
from torch import nn

from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.models import layers as L
from comfyui_parallelanything_amd.models import sd_unet as U
from comfyui_parallelanything_amd.models import wan as W

BF16, F16, F32, F64 = (torch.bfloat16, torch.float16, torch.float32,
                       torch.float64)
DTYPES16 = (BF16, F16)

# limit = M * e_ref(tap). Two conditions (docs/KERNELS.md, "Block
# composition"): (a) every fault in FAULTS exceeds 2 * M * e_ref at its tap
# (the weakest, softmax scale x 1.02, is 2.78 x e_ref in bf16 and 21.9 in
# fp16); (b) M >= 1.15 * the largest e_gpu / e_ref measured on the MI355X,
# 1.15 being attention_cases.RHO_MARGIN. Measured: 1.149 in bf16 and 1.994
# in fp16, both at the ResBlock's output (MIOpen's convolution; the
# transformer blocks stay under 1.12 and 1.13), 1.495 in fp32, and 1.129 /
# 1.846 for the whole models (SD1.5, the same convolutions).
M = {BF16: 1.33, F16: 2.3}
# fp32 blocks on the GPU (attention on the reference path, fp32 norm
# kernels, _addmm_activation / addmm GEMM epilogues) against the CPU fp32 run
M32 = 2.0
# whole models: e_ref is the CPU 16-bit forward's distance from fp64
M_MODEL = {BF16: 1.35, F16: 2.2}
FAULT_FACTOR = 2.0      # a fault must exceed FAULT_FACTOR * limit
FP64_AGREE = 1e-9       # the two fp64 references, at every tap

# the ops attributes the blocks call (through the module: ops.<name>)
RECORDED = ("layer_norm_mod", "pack_joint_qkv", "qk_norm_rope_",
            "attention_bshd", "attention_bshd_split", "gate_residual",
            "group_norm_silu", "rms_norm", "gelu_tanh")

T_TXT = 37                  # text / context tokens
TXT_LENS = (5, 30)          # live text tokens per batch element
IMG_HW = (16, 17)           # 272 image tokens: S = 309, two query blocks
WAN_GRID = (7, 6, 8)        # 7 frames of 48 tokens: S = 336
SD_HW = (17, 16)            # 272 tokens
BATCH = 2
# Inputs are N(0, 1) but for two, chosen so that the faults can show:
# cross-attention has no qk-norm, so its logit spread comes from the inputs.
# N(0, 1) context through default-initialised projections gives logits of
# std 0.33 over the keys, a nearly uniform softmax on which no softmax scale
# shows; 3.5 gives std 1.15, what the qk-normed self-attention has here.
CONTEXT_STD = 3.5
# WAN's time modulation e: the std of Modulation(vec) in the MMDiT cases.
# A larger shift is a component every token shares, which flattens the
# self-attention after qk-norm.
MOD_STD = 0.3


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    """|a - b| / |b| in fp64 on the CPU (|a - b| where b is all zero)."""
    a = a.detach().to("cpu", F64)
    b = b.detach().to("cpu", F64)
    d, n = (a - b).norm().item(), b.norm().item()
    return d / n if n > 0 else d


# ---------------------------------------------------------------------------
# Recorder
# ---------------------------------------------------------------------------

class Recorder:
    """Replaces the RECORDED attributes of ``ops`` for one forward and keeps
    a clone of every result as ``<op>#<call index>[<output index>]``; the
    in-place qk_norm_rope_ is tapped as (q, k) after the call. Calls an op
    makes to another recorded op (the reference path of pack_joint_qkv and
    attention_bshd_split does) are not taps, so a CPU and a GPU run name the
    same taps. ``hook(name, index, args, kwargs) -> (args, kwargs)`` may
    change a call's arguments: the injected faults."""

    def __init__(self, hook: Optional[Callable] = None):
        self.taps = {}
        self.calls = {}
        self.hook = hook
        self._depth = 0

    def _wrap(self, name, orig):
        def wrapper(*args, **kwargs):
            if self._depth:
                return orig(*args, **kwargs)
            idx = self.calls.get(name, 0)
            self.calls[name] = idx + 1
            if self.hook is not None:
                args, kwargs = self.hook(name, idx, args, kwargs)
            self._depth += 1
            try:
                out = orig(*args, **kwargs)
            finally:
                self._depth -= 1
            if name == "qk_norm_rope_":
                outs = (args[0], args[1])
            else:
                outs = out if isinstance(out, (tuple, list)) else (out,)
            for j, t in enumerate(outs):
                self.taps[f"{name}#{idx}[{j}]"] = t.detach().clone()
            return out
        return wrapper

    def final(self, out):
        outs = out if isinstance(out, (tuple, list)) else (out,)
        for j, t in enumerate(outs):
            self.taps[f"out[{j}]"] = t.detach().clone()

    @contextlib.contextmanager
    def installed(self):
        saved = {name: getattr(ops, name) for name in RECORDED}
        try:
            for name, orig in saved.items():
                setattr(ops, name, self._wrap(name, orig))
            yield self
        finally:
            for name, orig in saved.items():
                setattr(ops, name, orig)


# ---------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    kind: str                   # double single wan last sdtx res
    width: int
    heads: int
    axes: Optional[Tuple[int, ...]] = None
    masked: bool = False        # key mask from TXT_LENS
    banked: bool = False        # mods from a ModulationBank over two blocks
    window: Optional[int] = None    # WAN frame window
    txt: int = T_TXT            # text / context tokens

    @property
    def id(self) -> str:
        s = f"{self.kind}-w{self.width}-D{self.width // self.heads}"
        s += "-masked" if self.masked else ""
        s += "-banked" if self.banked else ""
        s += f"-win{self.window}" if self.window is not None else ""
        s += f"-T{self.txt}" if self.txt != T_TXT else ""
        return s


_MMDIT_GEOM = ((256, 2, (16, 56, 56)), (128, 2, (16, 24, 24)))
_WAN_GEOM = ((256, 2, (44, 42, 42)), (128, 2, (16, 24, 24)))

CASES = tuple(
    [Case(kind, w, h, ax, masked, banked)
     for kind in ("double", "single")
     for (w, h, ax) in _MMDIT_GEOM
     for masked in (True, False) for banked in (True, False)]
    + [Case("wan", w, h, ax, True, False, window)
       for (w, h, ax) in _WAN_GEOM for window in (None, 1)]
    + [Case("last", 256, 2), Case("last", 128, 2)]
    + [Case("sdtx", 320, 8, None, True), Case("sdtx", 128, 2, None, True)]
    + [Case("res", 64, 1)])

COMPOSED_KINDS = ("double", "single", "wan", "last", "sdtx", "res")
MLP_KINDS = ("double", "single", "wan")     # blocks with a tanh-GELU MLP


def cases(*kinds):
    return [c for c in CASES if c.kind in kinds] if kinds else list(CASES)


@dataclass
class Built:
    case: Case
    modules: nn.ModuleList      # fp64 holders of values rounded to `dtype`
    inputs: dict                # fp64 tensors rounded to `dtype`; pe too
    dtype: torch.dtype


def _make_blocks(case: Case) -> nn.ModuleList:
    w, h = case.width, case.heads
    if case.kind == "double":
        return nn.ModuleList(L.DoubleStreamBlock(w, h) for _ in range(2))
    if case.kind == "single":
        return nn.ModuleList(L.SingleStreamBlock(w, h) for _ in range(2))
    if case.kind == "wan":
        return nn.ModuleList([W.WanBlock(w, 4 * w, h, w)])
    if case.kind == "last":
        return nn.ModuleList([L.LastLayer(w, 16)])
    if case.kind == "sdtx":
        return nn.ModuleList([U.TransformerBlock(w, 96, h)])
    if case.kind == "res":
        return nn.ModuleList([U.ResBlock(64, 128, 32)])
    raise ValueError(case.kind)


_BUILT = {}


def build(case: Case, dtype: torch.dtype) -> Built:
    """The case's blocks and inputs, every value representable in ``dtype``
    and held in fp64. Cached: callers copy, never change."""
    key = (case, dtype)
    if key in _BUILT:
        return _BUILT[key]
    seed = zlib.crc32(case.id.encode())
    g = torch.Generator(device="cpu").manual_seed(seed)

    def randn(*shape, s=1.0):
        return torch.randn(*shape, generator=g) * s

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed + 1)
        mods = _make_blocks(case).eval()
    with torch.no_grad():
        for name, p in mods.named_parameters():
            if name.endswith(".scale"):     # every RMSNorm weight
                p.copy_(1.0 + 0.5 * randn(*p.shape))
            if case.kind == "res" and ("norm.weight" in name
                                       or "norm.bias" in name):
                p.copy_((1.0 if name.endswith("weight") else 0.0)
                        + 0.5 * randn(*p.shape))
    B, w = BATCH, case.width
    inp = {}
    if case.kind in ("double", "single"):
        ih, iw = IMG_HW
        inp["img"] = randn(B, ih * iw, w)
        inp["txt"] = randn(B, case.txt, w)
        inp["vec"] = randn(B, w)
        inp["pe"] = L.rope_2d_table(ih, iw, case.axes, text_len=case.txt)
    elif case.kind == "wan":
        f, gh, gw = WAN_GRID
        inp["x"] = randn(B, f * gh * gw, w)
        inp["e"] = randn(B, 6, w, s=MOD_STD)
        inp["context"] = randn(B, case.txt, w, s=CONTEXT_STD)
        inp["pe"] = W.rope_3d_table(f, gh, gw, case.axes, 10000.0, "cpu")
    elif case.kind == "last":
        inp["x"] = randn(B, IMG_HW[0] * IMG_HW[1], w)
        inp["vec"] = randn(B, w)
    elif case.kind == "sdtx":
        inp["x"] = randn(B, SD_HW[0] * SD_HW[1], w)
        inp["context"] = randn(B, case.txt, 96, s=CONTEXT_STD)
    elif case.kind == "res":
        inp["x"] = randn(B, 64, 9, 7)
        inp["emb"] = randn(B, 32)
    mods = mods.to(dtype).double()
    inp = {k: v.to(dtype).double() for k, v in inp.items()}
    _BUILT[key] = Built(case, mods, inp, dtype)
    return _BUILT[key]


def text_mask(device="cpu", lens=TXT_LENS, T=T_TXT) -> torch.Tensor:
    """[B, T] bool attention_mask, ``lens`` live tokens per element."""
    return (torch.arange(T, device=device)[None, :]
            < torch.tensor(lens, device=device)[:, None])


@dataclass
class Fault:
    """One injected wiring fault, run in fp64: any of a change to a copy of
    the blocks (``mutate(modules)``), to the block's keyword arguments
    (``inputs(kw, ctx)``, ctx holding the bank's results and the device) or
    to one op call's arguments (``hook``, see Recorder). ``taps`` names the
    taps at which the fault must exceed FAULT_FACTOR * limit (one of them
    is enough); ``fp32_only`` faults are below 16-bit rounding and are held
    by the fp32 limits instead. ``refused`` declares that a later op
    refuses the faulted forward with a RuntimeError (a split point off by
    one leaves gate_residual two shapes that do not match): the run then
    keeps the taps up to the refusal. Any other error of a faulted run is
    an error of the test."""
    name: str
    kinds: Tuple[str, ...]
    taps: Tuple[str, ...]
    mutate: Optional[Callable] = None
    inputs: Optional[Callable] = None
    hook: Optional[Callable] = None
    needs: Optional[Callable] = None    # case -> bool
    fp32_only: bool = False
    refused: bool = False

    def applies(self, case: Case) -> bool:
        return case.kind in self.kinds and (self.needs is None
                                            or self.needs(case))


def call_kwargs(built: Built, modules, device, dtype, fault=None) -> dict:
    """The block's arguments on ``device`` in ``dtype``; masks and banked
    modulation are made there by the models' own helpers."""
    case = built.case
    inp = {k: v.to(device, dtype) for k, v in built.inputs.items()}
    if "pe" in inp:     # the models keep the table in fp32
        inp["pe"] = built.inputs["pe"].to(device,
                                          F64 if dtype == F64 else F32)
    B = BATCH
    ctx = {"device": device, "dtype": dtype, "banked": None}
    if case.kind == "double":
        kw = dict(img=inp["img"], txt=inp["txt"], vec=inp["vec"],
                  pe=inp["pe"], mods=None, key_mask=None)
        if case.banked:
            bank = L.ModulationBank([modules[0].img_mod, modules[0].txt_mod,
                                     modules[1].img_mod, modules[1].txt_mod])
            ctx["banked"] = bank(inp["vec"])
            kw["mods"] = (ctx["banked"][0], ctx["banked"][1])
    elif case.kind == "single":
        kw = dict(x=torch.cat([inp["txt"], inp["img"]], dim=1),
                  vec=inp["vec"], pe=inp["pe"], mods=None, key_mask=None)
        if case.banked:
            bank = L.ModulationBank([modules[0].modulation,
                                     modules[1].modulation])
            ctx["banked"] = bank(inp["vec"])
            kw["mods"] = (ctx["banked"][0][0],)
    elif case.kind == "wan":
        kw = dict(x=inp["x"], e=inp["e"], context=inp["context"],
                  pe=inp["pe"], key_mask=None, block_mask=None)
        if case.window is not None:
            f, gh, gw = WAN_GRID
            S = f * gh * gw
            kw["block_mask"] = ops.pack_block_mask(
                ops.frame_window_block_mask(f, gh * gw, case.window,
                                            device=device), B, S, S)
    elif case.kind == "last":
        kw = dict(x=inp["x"], vec=inp["vec"])
    elif case.kind == "sdtx":
        kw = dict(x=inp["x"], context=inp["context"], key_mask=None)
    elif case.kind == "res":
        kw = dict(x=inp["x"], emb=inp["emb"])
    if case.masked:
        am = text_mask(device, T=case.txt)
        if case.kind in ("double", "single"):
            kw["key_mask"] = L.joint_key_mask(am, B, case.txt,
                                              IMG_HW[0] * IMG_HW[1])
        else:
            kw["key_mask"] = L.context_key_mask(am, inp["context"])
    if fault is not None and fault.inputs is not None:
        kw = fault.inputs(dict(kw), ctx)
    return kw


def run(built: Built, device="cpu", dtype=F64, fault: Optional[Fault] = None,
        kw_edit: Optional[Callable] = None) -> dict:
    """One recorded forward of the case's block: {tap name: tensor} on
    ``device``. ``kw_edit(kw)`` may change the arguments (the exact-property
    tests). A fault that declares ``refused`` must end in a RuntimeError
    and keeps the taps up to it."""
    modules = copy.deepcopy(built.modules)
    if fault is not None and fault.mutate is not None:
        with torch.no_grad():
            fault.mutate(modules)
    modules = modules.to(device=device, dtype=dtype).eval()
    rec = Recorder(fault.hook if fault is not None else None)
    with torch.no_grad():
        kw = call_kwargs(built, modules, device, dtype, fault)
        if kw_edit is not None:
            kw = kw_edit(kw)
        with rec.installed():
            if fault is not None and fault.refused:
                try:
                    modules[0](**kw)
                except RuntimeError:
                    return rec.taps
                raise AssertionError(f"{fault.name}: no op refused the run")
            rec.final(modules[0](**kw))
    return rec.taps


def errors(taps: dict, ref: dict) -> dict:
    """rel-l2 of every tap from the fp64 taps ``ref``; the two runs must
    have made the same calls."""
    assert list(taps) == list(ref), (
        f"taps differ: {sorted(set(taps) ^ set(ref))}")
    return {name: rel_l2(t, ref[name]) for name, t in taps.items()}


# ---------------------------------------------------------------------------
# The second fp64 reference: every block written out with torch arithmetic
# only (no ops.* and no reference.* call; the convolutions of the ResBlock
# are torch's). The masks are written out too, from TXT_LENS and the frame
# arithmetic, not taken from the models' helpers.
# ---------------------------------------------------------------------------

def _silu(x):
    return x / (1.0 + torch.exp(-x))


def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(
        math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


def _lin(x, lin):
    y = x @ lin.weight.t()
    return y if lin.bias is None else y + lin.bias


def _ln(x, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps)


def _ln_mod(x, scale, shift):
    return _ln(x, 1e-6) * (1.0 + scale[:, None, :]) + shift[:, None, :]


def _rms(x, w):
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + 1e-6) * w


def _rot(x, cs):
    """x [B, S, H, D], cs [S, D/2, 2]: rotate the adjacent pairs."""
    x0, x1 = x[..., 0::2], x[..., 1::2]
    c, s = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
    out = torch.empty_like(x)
    out[..., 0::2] = x0 * c - x1 * s
    out[..., 1::2] = x0 * s + x1 * c
    return out


def _attn(q, k, v, scale, vis=None):
    """[B, S, H, D]; vis: bool, broadcastable to [B, Sq, Sk], True = the
    query row sees the key."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    if vis is not None:
        s = s.masked_fill(~vis[:, None].expand(s.shape[0], 1, *s.shape[2:]),
                          float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    return torch.einsum("bhqk,bkhd->bqhd", p, v)


def _mod_chunks(mod, vec):
    dim = vec.shape[-1]
    out = _lin(_silu(vec), mod.lin)
    return [out[:, i * dim:(i + 1) * dim] for i in range(mod.multiplier)]


def _key_vis(case, n_img=0):
    """[B, 1, Sk] bool: text key j of element b is live iff j < TXT_LENS[b];
    the n_img image keys after the text are all live. None: no mask."""
    if not case.masked:
        return None
    vis = torch.zeros(BATCH, 1, case.txt + n_img, dtype=torch.bool)
    for b, n in enumerate(TXT_LENS):
        vis[b, 0, :n] = True
    vis[:, :, case.txt:] = True
    return vis


def _window_vis(case):
    """[1, S, S] bool: query row i sees key j iff some frame of j's 64-key
    tile lies within ``window`` frames of some frame of i's 256-row block."""
    if case.window is None:
        return None
    f, gh, gw = WAN_GRID
    tpf, S = gh * gw, f * gh * gw
    vis = torch.zeros(1, S, S, dtype=torch.bool)
    for q0 in range(0, S, 256):
        q1 = min(q0 + 256, S)
        for k0 in range(0, S, 64):
            k1 = min(k0 + 64, S)
            if ((k1 - 1) // tpf >= q0 // tpf - case.window
                    and k0 // tpf <= (q1 - 1) // tpf + case.window):
                vis[0, q0:q1, k0:k1] = True
    return vis


def _heads(x, H):
    return x.reshape(x.shape[0], x.shape[1], H, -1)


def _compose_double(blk, kw):
    img, txt, vec, pe = kw["img"], kw["txt"], kw["vec"], kw["pe"]
    T, H = txt.shape[1], blk.num_heads
    taps = {}
    ish1, isc1, ig1, ish2, isc2, ig2 = _mod_chunks(blk.img_mod, vec)
    tsh1, tsc1, tg1, tsh2, tsc2, tg2 = _mod_chunks(blk.txt_mod, vec)
    tn = taps["layer_norm_mod#0[0]"] = _ln_mod(txt, tsc1, tsh1)
    im = taps["layer_norm_mod#1[0]"] = _ln_mod(img, isc1, ish1)
    tq, tk, tv = _lin(tn, blk.txt_attn_qkv).reshape(
        *tn.shape[:2], 3, H, -1).unbind(2)
    iq, ik, iv = _lin(im, blk.img_attn_qkv).reshape(
        *im.shape[:2], 3, H, -1).unbind(2)
    tn_, in_ = blk.txt_attn_norm, blk.img_attn_norm
    q = _rot(torch.cat([_rms(tq, tn_.query_norm.scale),
                        _rms(iq, in_.query_norm.scale)], 1), pe)
    k = _rot(torch.cat([_rms(tk, tn_.key_norm.scale),
                        _rms(ik, in_.key_norm.scale)], 1), pe)
    v = torch.cat([tv, iv], 1)
    taps["pack_joint_qkv#0[0]"], taps["pack_joint_qkv#0[1]"] = q, k
    taps["pack_joint_qkv#0[2]"] = v
    a = _attn(q, k, v, 1.0 / math.sqrt(q.shape[-1]),
              _key_vis(kw["_case"], img.shape[1]))
    ta = taps["attention_bshd_split#0[0]"] = a[:, :T]
    ia = taps["attention_bshd_split#0[1]"] = a[:, T:]
    img = taps["gate_residual#0[0]"] = img + ig1[:, None] * _lin(
        ia.flatten(2), blk.img_attn_proj)
    h = taps["layer_norm_mod#2[0]"] = _ln_mod(img, isc2, ish2)
    img = taps["gate_residual#1[0]"] = img + ig2[:, None] * _lin(
        _gelu_tanh(_lin(h, blk.img_mlp.up.lin)), blk.img_mlp.down)
    txt = taps["gate_residual#2[0]"] = txt + tg1[:, None] * _lin(
        ta.flatten(2), blk.txt_attn_proj)
    h = taps["layer_norm_mod#3[0]"] = _ln_mod(txt, tsc2, tsh2)
    txt = taps["gate_residual#3[0]"] = txt + tg2[:, None] * _lin(
        _gelu_tanh(_lin(h, blk.txt_mlp.up.lin)), blk.txt_mlp.down)
    taps["out[0]"], taps["out[1]"] = img, txt
    return taps


def _compose_single(blk, kw):
    x, vec, pe = kw["x"], kw["vec"], kw["pe"]
    H = blk.num_heads
    taps = {}
    shift, scale, gate = _mod_chunks(blk.modulation, vec)
    xn = taps["layer_norm_mod#0[0]"] = _ln_mod(x, scale, shift)
    q, k, v = _lin(xn, blk.linear1_qkv).reshape(
        *xn.shape[:2], 3, H, -1).unbind(2)
    q = taps["qk_norm_rope_#0[0]"] = _rot(
        _rms(q, blk.norm.query_norm.scale), pe)
    k = taps["qk_norm_rope_#0[1]"] = _rot(
        _rms(k, blk.norm.key_norm.scale), pe)
    a = taps["attention_bshd#0[0]"] = _attn(
        q, k, v, 1.0 / math.sqrt(q.shape[-1]),
        _key_vis(kw["_case"], x.shape[1] - kw["_case"].txt))
    out = _lin(a.flatten(2), blk.linear2_attn) + _lin(
        _gelu_tanh(_lin(xn, blk.linear1_mlp.lin)), blk.linear2_mlp)
    y = taps["gate_residual#0[0]"] = x + gate[:, None] * out
    taps["out[0]"] = y
    return taps


def _compose_wan(blk, kw):
    x, e, ctx, pe = kw["x"], kw["e"], kw["context"], kw["pe"]
    H = blk.num_heads
    sc = 1.0 / math.sqrt(x.shape[-1] // H)
    taps = {}
    m = e + blk.mod
    sh1, sc1, g1, sh2, sc2, g2 = (m[:, i] for i in range(6))
    xn = taps["layer_norm_mod#0[0]"] = _ln_mod(x, sc1, sh1)
    q, k, v = _lin(xn, blk.self_qkv).reshape(
        *xn.shape[:2], 3, H, -1).unbind(2)
    q = taps["qk_norm_rope_#0[0]"] = _rot(
        _rms(q, blk.self_norm.query_norm.scale), pe)
    k = taps["qk_norm_rope_#0[1]"] = _rot(
        _rms(k, blk.self_norm.key_norm.scale), pe)
    a = taps["attention_bshd#0[0]"] = _attn(q, k, v, sc,
                                            _window_vis(kw["_case"]))
    x = taps["gate_residual#0[0]"] = x + g1[:, None] * _lin(
        a.flatten(2), blk.self_proj)
    h = _ln(x, blk.norm_cross.eps) * blk.norm_cross.weight \
        + blk.norm_cross.bias
    a = taps["attention_bshd#1[0]"] = _attn(
        _heads(_lin(h, blk.cross_q), H), _heads(_lin(ctx, blk.cross_k), H),
        _heads(_lin(ctx, blk.cross_v), H), sc, _key_vis(kw["_case"]))
    x = x + _lin(a.flatten(2), blk.cross_proj)
    h = taps["layer_norm_mod#1[0]"] = _ln_mod(x, sc2, sh2)
    x = taps["gate_residual#1[0]"] = x + g2[:, None] * _lin(
        _gelu_tanh(_lin(h, blk.ffn.up.lin)), blk.ffn.down)
    taps["out[0]"] = x
    return taps


def _compose_last(blk, kw):
    x, vec = kw["x"], kw["vec"]
    dim = vec.shape[-1]
    ada = _lin(_silu(vec), blk.ada_lin)
    shift, scale = ada[:, :dim], ada[:, dim:]
    taps = {}
    h = taps["layer_norm_mod#0[0]"] = _ln_mod(x, scale, shift)
    taps["out[0]"] = _lin(h, blk.linear)
    return taps


def _compose_sdtx(blk, kw):
    x, ctx = kw["x"], kw["context"]
    taps = {}

    def ln(x, n):
        return _ln(x, n.eps) * n.weight + n.bias

    def attn(a, xq, xk, vis):
        H = a.num_heads
        return _attn(_heads(_lin(xq, a.to_q), H), _heads(_lin(xk, a.to_k), H),
                     _heads(_lin(xk, a.to_v), H),
                     1.0 / math.sqrt(xq.shape[-1] // H), vis)

    h = ln(x, blk.norm1)
    a = taps["attention_bshd#0[0]"] = attn(blk.attn1, h, h, None)
    x = x + _lin(a.flatten(2), blk.attn1.to_out)
    a = taps["attention_bshd#1[0]"] = attn(blk.attn2, ln(x, blk.norm2), ctx,
                                           _key_vis(kw["_case"]))
    x = x + _lin(a.flatten(2), blk.attn2.to_out)
    p = _lin(ln(x, blk.norm3), blk.ff[0].proj)
    half = p.shape[-1] // 2
    u, g = p[..., :half], p[..., half:]
    g = 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))     # erf-GELU
    taps["out[0]"] = x + _lin(u * g, blk.ff[1])
    return taps


def _gn_silu(x, n):
    B, C, H, W = x.shape
    xg = x.reshape(B, n.groups, -1)
    mu = xg.mean(-1, keepdim=True)
    var = ((xg - mu) ** 2).mean(-1, keepdim=True)
    y = ((xg - mu) / torch.sqrt(var + 1e-6)).reshape(B, C, H, W)
    return _silu(y * n.weight[None, :, None, None]
                 + n.bias[None, :, None, None])


def _compose_res(blk, kw):
    x, emb = kw["x"], kw["emb"]
    conv = torch.nn.functional.conv2d
    taps = {}
    h = taps["group_norm_silu#0[0]"] = _gn_silu(x, blk.in_norm)
    h = conv(h, blk.conv1.weight, blk.conv1.bias, padding=1)
    h = h + _lin(_silu(emb), blk.emb_proj)[:, :, None, None]
    h = taps["group_norm_silu#1[0]"] = _gn_silu(h, blk.out_norm)
    h = conv(h, blk.conv2.weight, blk.conv2.bias, padding=1)
    taps["out[0]"] = conv(x, blk.skip.weight, blk.skip.bias) + h
    return taps


_COMPOSE = {"double": _compose_double, "single": _compose_single,
            "wan": _compose_wan, "last": _compose_last,
            "sdtx": _compose_sdtx, "res": _compose_res}


def compose(built: Built) -> dict:
    """The case's taps from the written-out fp64 composition. The banked
    cases compute the modulation from the block's own Modulation weights,
    and every mask is built here from the case, so the bank's slices and
    the models' mask helpers are checked too."""
    modules = copy.deepcopy(built.modules).double()
    with torch.no_grad():
        kw = call_kwargs(built, modules, "cpu", F64)
        for name in ("key_mask", "block_mask", "mods"):
            kw.pop(name, None)      # written out from the case instead
        kw["_case"] = built.case
        return _COMPOSE[built.case.kind](modules[0], kw)


_REF = {}


def reference(built: Built) -> dict:
    """The fp64 taps of the module itself (``.double()`` on the CPU
    reference path), computed once per case and dtype and never changed."""
    key = (built.case, built.dtype)
    if key not in _REF:
        _REF[key] = run(built, "cpu", F64)
    return _REF[key]


_EREF = {}


def e_ref(built: Built, dtype=None) -> dict:
    """rel-l2 per tap of the CPU run in ``dtype`` (default: the case's
    16-bit type) from fp64: the yardstick."""
    dtype = dtype or built.dtype
    key = (built.case, built.dtype, dtype)
    if key not in _EREF:
        _EREF[key] = errors(run(built, "cpu", dtype), reference(built))
    return _EREF[key]


# ---------------------------------------------------------------------------
# Faults
# ---------------------------------------------------------------------------

def _arg_hook(op, index, edit):
    """A Recorder hook that edits call ``index`` (None: every call) of
    ``op``: edit(args list, kwargs dict) changes them in place."""
    def hook(name, idx, args, kwargs):
        if name == op and (index is None or idx == index):
            args, kwargs = list(args), dict(kwargs)
            edit(args, kwargs)
            args = tuple(args)
        return args, kwargs
    return hook


def _swap(i, j):
    def edit(args, kwargs):
        args[i], args[j] = args[j], args[i]
    return edit


def _shift_rows(i):
    def edit(args, kwargs):
        cs = args[i]
        args[i] = torch.cat([cs[1:], cs[-1:]], dim=0)
    return edit


def _scale_by(i, factor):
    def edit(args, kwargs):
        args[i] = args[i] * factor
    return edit


def _lens_mask(delta):
    """The key mask with every element's text length changed by delta."""
    def edit(args, kwargs):
        km = kwargs["key_mask"]
        m = km.mask.clone()
        m[:, :T_TXT] = text_mask(m.device,
                                 tuple(n + delta for n in TXT_LENS))
        kwargs["key_mask"] = ops.pack_key_mask(m)
    return edit


def _drop_mask(args, kwargs):
    kwargs["key_mask"] = None


def _split_by(delta):
    def edit(args, kwargs):
        args[3] = args[3] + delta
    return edit


def _swap_mod_rows(mod, a, b):
    """Exchange chunks a and b of a Modulation's projection."""
    dim = mod.lin.in_features
    for p in (mod.lin.weight, mod.lin.bias):
        ra, rb = p[a * dim:(a + 1) * dim].clone(), p[b * dim:(b + 1) * dim].clone()
        p[a * dim:(a + 1) * dim], p[b * dim:(b + 1) * dim] = rb, ra


def _erf_gelu(gl):
    gl.forward = lambda x: torch.nn.functional.gelu(gl.lin(x))


def _window(w):
    def inputs(kw, ctx):
        f, gh, gw = WAN_GRID
        S = f * gh * gw
        kw["block_mask"] = ops.pack_block_mask(
            ops.frame_window_block_mask(f, gh * gw, w, device=ctx["device"]),
            BATCH, S, S)
        return kw
    return inputs


def _wan_other_gate(kw, ctx):
    kw["e"] = kw["e"][:, [0, 1, 5, 3, 4, 2]]
    return kw


def _wan_other_gate_mod(ms):
    ms[0].mod.copy_(ms[0].mod[:, [0, 1, 5, 3, 4, 2]])


def _neighbour_bank(kind):
    def inputs(kw, ctx):
        b = ctx["banked"]
        kw["mods"] = (b[2], b[3]) if kind == "double" else (b[1][0],)
        return kw
    return inputs


_masked = lambda c: c.masked                                    # noqa: E731
_banked = lambda c: c.banked                                    # noqa: E731
_windowed = lambda c: c.window is not None                      # noqa: E731
_D = ("double",)
_S = ("single",)
_SW = ("single", "wan")

_Q, _K = "pack_joint_qkv#0[0]", "pack_joint_qkv#0[1]"
_AT, _AI = "attention_bshd_split#0[0]", "attention_bshd_split#0[1]"
_SQ, _SK, _SA = ("qk_norm_rope_#0[0]", "qk_norm_rope_#0[1]",
                 "attention_bshd#0[0]")

FAULTS = (
    # --- DoubleStreamBlock
    Fault("rotary rows shifted by one", _D, (_Q, _K),
          hook=_arg_hook("pack_joint_qkv", 0, _shift_rows(6))),
    Fault("mask one key short", _D, (_AT, _AI), needs=_masked,
          hook=_arg_hook("attention_bshd_split", 0, _lens_mask(-1))),
    Fault("mask one key long", _D, (_AT, _AI), needs=_masked,
          hook=_arg_hook("attention_bshd_split", 0, _lens_mask(+1))),
    Fault("mask dropped", _D, (_AT, _AI), needs=_masked,
          hook=_arg_hook("attention_bshd_split", 0, _drop_mask)),
    Fault("softmax scale x 1.02", _D, (_AT, _AI),
          hook=_arg_hook("attention_bshd_split", 0, _scale_by(4, 1.02))),
    Fault("txt/img k-norm weights swapped", _D, (_K,),
          hook=_arg_hook("pack_joint_qkv", 0, _swap(3, 5))),
    Fault("txt/img q-norm weights swapped", _D, (_Q,),
          hook=_arg_hook("pack_joint_qkv", 0, _swap(2, 4))),
    Fault("img q/k norm weights swapped", _D, (_Q, _K),
          hook=_arg_hook("pack_joint_qkv", 0, _swap(4, 5))),
    Fault("txt q/k norm weights swapped", _D, (_Q, _K),
          hook=_arg_hook("pack_joint_qkv", 0, _swap(2, 3))),
    Fault("split point T + 1", _D, (_AT, _AI),
          hook=_arg_hook("attention_bshd_split", 0, _split_by(+1)),
          refused=True),
    Fault("split point T - 1", _D, (_AT, _AI),
          hook=_arg_hook("attention_bshd_split", 0, _split_by(-1)),
          refused=True),
    Fault("shift and scale exchanged (txt LN 1)", _D, ("layer_norm_mod#0[0]",),
          hook=_arg_hook("layer_norm_mod", 0, _swap(1, 2))),
    Fault("shift and scale exchanged (img LN 2)", _D, ("layer_norm_mod#2[0]",),
          hook=_arg_hook("layer_norm_mod", 2, _swap(1, 2))),
    Fault("img gate from the other modulation set", _D,
          ("gate_residual#0[0]", "gate_residual#1[0]"),
          mutate=lambda ms: _swap_mod_rows(ms[0].img_mod, 2, 5)),
    Fault("txt gate from the other modulation set", _D,
          ("gate_residual#2[0]", "gate_residual#3[0]"),
          mutate=lambda ms: _swap_mod_rows(ms[0].txt_mod, 2, 5)),
    Fault("bank entry of the neighbouring block", _D,
          ("layer_norm_mod#0[0]", "layer_norm_mod#1[0]"), needs=_banked,
          inputs=_neighbour_bank("double")),
    # 1.8e-4 of the branch, far below 16-bit rounding: held by the fp32
    # limits (M32), not by the 16-bit ones
    Fault("erf-GELU for tanh-GELU (img MLP)", _D, ("gate_residual#1[0]",),
          mutate=lambda ms: _erf_gelu(ms[0].img_mlp.up), fp32_only=True),
    # --- SingleStreamBlock and WanBlock self-attention
    Fault("rotary rows shifted by one", _SW, (_SQ, _SK),
          hook=_arg_hook("qk_norm_rope_", 0, _shift_rows(4))),
    Fault("q/k norm weights swapped", _SW, (_SQ, _SK),
          hook=_arg_hook("qk_norm_rope_", 0, _swap(2, 3))),
    Fault("softmax scale x 1.02", _SW, (_SA,),
          hook=_arg_hook("attention_bshd", 0, _scale_by(3, 1.02))),
    Fault("shift and scale exchanged", _SW, ("layer_norm_mod#0[0]",),
          hook=_arg_hook("layer_norm_mod", 0, _swap(1, 2))),
    Fault("mask one key short", _S, (_SA,), needs=_masked,
          hook=_arg_hook("attention_bshd", 0, _lens_mask(-1))),
    Fault("mask one key long", _S, (_SA,), needs=_masked,
          hook=_arg_hook("attention_bshd", 0, _lens_mask(+1))),
    Fault("mask dropped", _S, (_SA,), needs=_masked,
          hook=_arg_hook("attention_bshd", 0, _drop_mask)),
    Fault("gate from the shift chunk", _S, ("gate_residual#0[0]",),
          mutate=lambda ms: _swap_mod_rows(ms[0].modulation, 0, 2)),
    Fault("bank entry of the neighbouring block", _S,
          ("layer_norm_mod#0[0]",), needs=_banked,
          inputs=_neighbour_bank("single")),
    Fault("erf-GELU for tanh-GELU", _S, ("gate_residual#0[0]",),
          mutate=lambda ms: _erf_gelu(ms[0].linear1_mlp), fp32_only=True),
    # --- WanBlock
    Fault("cross mask one key short", ("wan",), ("attention_bshd#1[0]",),
          hook=_arg_hook("attention_bshd", 1, _lens_mask(-1))),
    Fault("cross mask one key long", ("wan",), ("attention_bshd#1[0]",),
          hook=_arg_hook("attention_bshd", 1, _lens_mask(+1))),
    Fault("cross mask dropped", ("wan",), ("attention_bshd#1[0]",),
          hook=_arg_hook("attention_bshd", 1, _drop_mask)),
    Fault("cross softmax scale x 1.02", ("wan",), ("attention_bshd#1[0]",),
          hook=_arg_hook("attention_bshd", 1, _scale_by(3, 1.02))),
    Fault("frame window W + 1", ("wan",), (_SA,), needs=_windowed,
          inputs=_window(2)),
    Fault("frame window W - 1", ("wan",), (_SA,), needs=_windowed,
          inputs=_window(0)),
    Fault("frame window dropped", ("wan",), (_SA,), needs=_windowed,
          inputs=lambda kw, ctx: {**kw, "block_mask": None}),
    Fault("gate from the other modulation set", ("wan",),
          ("gate_residual#0[0]", "gate_residual#1[0]"),
          inputs=_wan_other_gate, mutate=_wan_other_gate_mod),
    Fault("self.mod bias left out", ("wan",), ("layer_norm_mod#0[0]",),
          mutate=lambda ms: ms[0].mod.zero_()),
    Fault("erf-GELU for tanh-GELU", ("wan",), ("gate_residual#1[0]",),
          mutate=lambda ms: _erf_gelu(ms[0].ffn.up), fp32_only=True),
    # --- sd_unet.TransformerBlock (its FF is an erf-GELU GEGLU by design)
    Fault("cross mask one key short", ("sdtx",), ("attention_bshd#1[0]",),
          hook=_arg_hook("attention_bshd", 1, _lens_mask(-1))),
    Fault("cross mask one key long", ("sdtx",), ("attention_bshd#1[0]",),
          hook=_arg_hook("attention_bshd", 1, _lens_mask(+1))),
    Fault("cross mask dropped", ("sdtx",), ("attention_bshd#1[0]",),
          hook=_arg_hook("attention_bshd", 1, _drop_mask)),
    Fault("self softmax scale x 1.02", ("sdtx",), ("attention_bshd#0[0]",),
          hook=_arg_hook("attention_bshd", 0, _scale_by(3, 1.02))),
    Fault("cross softmax scale x 1.02", ("sdtx",), ("attention_bshd#1[0]",),
          hook=_arg_hook("attention_bshd", 1, _scale_by(3, 1.02))),
    # --- LastLayer
    Fault("shift and scale exchanged", ("last",), ("layer_norm_mod#0[0]",),
          hook=_arg_hook("layer_norm_mod", 0, _swap(1, 2))),
)


def faults_for(case: Case, fp32_only: bool = False):
    return [f for f in FAULTS
            if f.applies(case) and f.fp32_only == fp32_only]


def fault_distance(built: Built, fault: Fault) -> dict:
    """rel-l2 per tap of the faulted fp64 run from the clean fp64 run; inf
    where the fault changed the tap's shape."""
    ref = reference(built)
    return {name: (rel_l2(t, ref[name]) if t.shape == ref[name].shape
                   else math.inf)
            for name, t in run(built, "cpu", F64, fault).items()}


# ---------------------------------------------------------------------------
# Whole models at a real head dim (64 / 128) and the blocks' sequence
# ---------------------------------------------------------------------------

def _flux(**over):
    from comfyui_parallelanything_amd.models.mmdit import Flux, FluxConfig
    kw = dict(in_channels=4, hidden=256, num_heads=2, depth_double=2,
              depth_single=2, context_dim=32, vec_dim=16,
              axes_dim=(16, 56, 56), time_embed_dim=32)
    kw.update(over)
    return Flux(FluxConfig(**kw))


def _zimage():
    from comfyui_parallelanything_amd.models.mmdit import ZImage, ZImageConfig
    return ZImage(ZImageConfig(in_channels=4, hidden=256, num_heads=2,
                               depth=2, context_dim=32,
                               axes_dim=(16, 56, 56), time_embed_dim=32))


def _wan(**over):
    kw = dict(in_channels=4, dim=256, ffn_dim=512, num_heads=2, depth=2,
              ctx_dim=32, axes_dim=(44, 42, 42), time_embed_dim=32)
    kw.update(over)
    return W.WanDiT(W.WanConfig(**kw))


def _sd15():
    return U.SDUNet(U.UNetConfig(
        model_channels=64, channel_mult=(1, 2), num_res_blocks=1,
        transformer_depth=(1, 1), context_dim=32, head_dim=64))


_IMG_LATENT = (BATCH, 4, 2 * IMG_HW[0], 2 * IMG_HW[1])      # 16 x 17 tokens
_VID_LATENT = (BATCH, 4, WAN_GRID[0], 2 * WAN_GRID[1], 2 * WAN_GRID[2])

# name -> (constructor, latent shape, extra inputs {name: shape})
MODEL_CASES = {
    "flux-D128": (_flux, _IMG_LATENT, {"y": (BATCH, 16)}),
    "sd3-D64": (lambda: _flux(hidden=128, depth_single=0,
                              axes_dim=(16, 24, 24), guidance_embed=False),
                _IMG_LATENT, {"y": (BATCH, 16)}),
    "zimage-D128": (_zimage, _IMG_LATENT, {}),
    "wan-D128": (_wan, _VID_LATENT, {}),
    "wan-D128-win1": (lambda: _wan(self_attn_frame_window=1), _VID_LATENT,
                      {}),
    "wan-i2v-D128": (lambda: _wan(cond_channels=5), _VID_LATENT,
                     {"image_cond": (BATCH, 5) + _VID_LATENT[2:]}),
    # 34 x 32 latent: 1088 tokens at 64 channels, 17 x 16 at 128
    "sd15-D64": (_sd15, (BATCH, 4, 34, 32), {}),
}

_MODELS = {}


def build_model(name: str, dtype: torch.dtype):
    """(model, inputs): fp64 holders of values rounded to ``dtype``; every
    ``*.scale`` norm weight is 1 + 0.5 randn. Cached: callers copy."""
    key = (name, dtype)
    if key in _MODELS:
        return _MODELS[key]
    make, latent, extra = MODEL_CASES[name]
    seed = zlib.crc32(name.encode())
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed + 1)
        model = make().eval()
    with torch.no_grad():
        for pname, p in model.named_parameters():
            if pname.endswith(".scale"):
                p.copy_(1.0 + 0.5 * torch.randn(*p.shape, generator=g))
    inp = {"x": torch.randn(*latent, generator=g),
           "context": torch.randn(BATCH, T_TXT, 32, generator=g)}
    for k, shape in extra.items():
        inp[k] = torch.randn(*shape, generator=g)
    inp = {k: v.to(dtype).double() for k, v in inp.items()}
    inp["timesteps"] = torch.rand(BATCH, generator=g)       # fp32, as served
    _MODELS[key] = (model.to(dtype).double(), inp)
    return _MODELS[key]


def run_model(name: str, values: torch.dtype, device="cpu", dtype=F64,
              prepare: Optional[Callable] = None) -> torch.Tensor:
    """One forward with ``attention_mask`` lengths TXT_LENS, on ``device``
    in ``dtype``. ``prepare(model)`` may change the copy's configuration."""
    master, inp = build_model(name, values)
    model = copy.deepcopy(master).to(device=device, dtype=dtype).eval()
    if prepare is not None:
        prepare(model)
    kw = {k: v.to(device, dtype) for k, v in inp.items()
          if k not in ("x", "timesteps")}
    with torch.no_grad():
        return model(inp["x"].to(device, dtype),
                     inp["timesteps"].to(device),
                     attention_mask=text_mask(device), **kw)


_MODEL_REF = {}


def model_reference(name: str, values: torch.dtype) -> torch.Tensor:
    key = (name, values)
    if key not in _MODEL_REF:
        _MODEL_REF[key] = run_model(name, values)
    return _MODEL_REF[key]


def model_e_ref(name: str, values: torch.dtype) -> float:
    """rel-l2 of the CPU forward in ``values`` (16-bit) from fp64."""
    return rel_l2(run_model(name, values, "cpu", values),
                  model_reference(name, values))
