"""Which extension binding each ops.attention* call reaches, and how: at the
head dim as it is, zero-padded to the tile class (64 / 128), or not at all
(the reference path, with its one-time note).

The numerics files pin what the kernels compute; this one pins the Python
dispatch above them, so the routing is checkable on its own. ROUTES is the
routing, written down once for the reader. Shapes are the smallest that
still cross a tile edge: Sq = 70 and Sk = 77 (one full 64-key tile and 13
keys), split at 7.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R
from test_gpu_attn_regimes import require_ext  # noqa: F401

B, H, SQ, SK, SPLIT = 1, 2, 70, 77, 7
DIMS = (40, 48, 64, 80, 96, 128, 160)

# The head dim the binding receives, per head dim of the call; None = no
# binding is reached. "keys" rows hold for no mask and for key_mask=, "block"
# rows for block_mask= (refused by the _lse ops: tested elsewhere).
#                                      D:  40    48    64   80    96    128  160
ROUTES = {
    ("attention", "keys"):             (40,   None, 64,  80,   None, 128, None),
    ("attention", "block"):            (None, None, 64,  None, None, 128, None),
    ("attention_bshd", "keys"):        (40,   64,   64,  80,   128,  128, None),
    ("attention_bshd", "block"):       (64,   64,   64,  128,  128,  128, None),
    # 64 and 128 reach the split bindings; every other head dim is
    # attention_bshd's route, sliced
    ("attention_bshd_split", "keys"):  (40,   64,   64,  80,   128,  128, None),
    ("attention_bshd_split", "block"): (64,   64,   64,  128,  128,  128, None),
    ("attention_lse", "keys"):         (None, None, 64,  None, None, 128, None),
    ("attention_bshd_lse", "keys"):    (64,   64,   64,  128,  128,  128, None),
}
BINDING = {"attention": "attn_fwd", "attention_bshd": "attn_fwd_bshd",
           "attention_bshd_split": "attn_fwd_bshd_split",
           "attention_lse": "attn_fwd_lse",
           "attention_bshd_lse": "attn_fwd_bshd_lse"}
CELLS = [(op, mask) for op in BINDING for mask in ("none", "keys", "block")
         if not (mask == "block" and op.endswith("_lse"))]


def expected(op, mask, D, dtype):
    """(bindings reached with the head dim each received, _unsupported
    keys)."""
    row = ROUTES[op, "block" if mask == "block" else "keys"]
    width = row[DIMS.index(D)] if dtype in C.DTYPES else None
    split = op == "attention_bshd_split"
    if width is not None:
        name = "attn_fwd_bshd" if split and D not in (64, 128) else BINDING[op]
        return [(name + ("_masked" if mask != "none" else ""), width)], set()
    why = f"dtype={dtype}, D={D}"
    if not split:
        return [], {(BINDING[op], why)}
    # attention_bshd's note, and the split op's own on unmasked calls only
    return [], {("attn_fwd_bshd", why)} | (
        {(BINDING[op], why)} if mask == "none" else set())


@pytest.fixture()
def spy(monkeypatch):
    """(calls, notes): every attn_fwd* call on the extension as (binding,
    last dim of q as received), passed through; every ops._unsupported key."""
    calls, notes = [], []
    ext = ops.hip_ext()

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(ext, name)
            if not name.startswith("attn_fwd"):
                return fn

            def forward(q, *args):
                calls.append((name, q.shape[-1]))
                return fn(q, *args)

            return forward

    orig = ops._unsupported

    def note(op, why):
        notes.append((op, why))
        return orig(op, why)

    monkeypatch.setattr(ops, "_EXT", Proxy())
    monkeypatch.setattr(ops, "_unsupported", note)
    return calls, notes


# built once, never modified
@functools.lru_cache(maxsize=None)
def _case(D, dtype):
    """[B, S, H, D] q, k, v on the device, a key mask with a hole in the
    full tile and a dead tail, a block mask that leaves the partial tile."""
    g = torch.Generator(device="cpu").manual_seed(D)
    q = torch.randn(B, SQ, H, D, generator=g).to(dtype).cuda()
    k = torch.randn(B, SK, H, D, generator=g).to(dtype).cuda()
    v = torch.randn(B, SK, H, D, generator=g).to(dtype).cuda()
    keys = torch.ones(B, SK, dtype=torch.bool)
    keys[:, 20:30] = False
    keys[:, 70:] = False
    block = torch.tensor([[False, True]])
    return (q, k, v), {"none": {}, "keys": dict(key_mask=keys.cuda()),
                       "block": dict(block_mask=block.cuda())}


@functools.lru_cache(maxsize=None)
def _reference(D, dtype, mask):
    """fp32 on the CPU, [B, S, H, D] and [B, S, H]."""
    qkv, masks = _case(D, dtype)
    out, lse = R.attention(
        *(t.float().cpu().permute(0, 2, 1, 3) for t in qkv), return_lse=True,
        **{n: m.cpu() for n, m in masks[mask].items()})
    return out.permute(0, 2, 1, 3), lse.permute(0, 2, 1)


def _padded_bshd(D, dtype, mask):
    """attention_bshd on q, k, v zero-padded to the tile class: what the
    native head dims and the pad route are both held to, bit for bit."""
    qkv, masks = _case(D, dtype)
    pad = (0, (64 if D <= 64 else 128) - D)
    return ops.attention_bshd(
        *(torch.nn.functional.pad(t, pad) for t in qkv), 1.0 / math.sqrt(D),
        **masks[mask])[..., :D]


def _check_route(op, mask, D, dtype, spy):
    calls, notes = spy
    qkv, masks = _case(D, dtype)
    bindings, keys = expected(op, mask, D, dtype)
    native = bool(bindings)
    # the comparison's other side first, then the call under test alone
    if not native:
        want = _reference(D, dtype, mask)[0]
    elif op == "attention_bshd":
        want = _padded_bshd(D, dtype, mask)
    else:
        want = ops.attention_bshd(*qkv, **masks[mask])
    del calls[:], notes[:]

    if op in ("attention", "attention_lse"):
        res = getattr(ops, op)(*(t.permute(0, 2, 1, 3) for t in qkv),
                               **masks[mask])
    elif op == "attention_bshd_split":
        res = ops.attention_bshd_split(*qkv, SPLIT, **masks[mask])
    else:
        res = getattr(ops, op)(*qkv, **masks[mask])
    what = f"{op} {mask} D={D} {dtype}"
    assert calls == bindings, what
    assert set(notes) == keys, what

    lse = None
    if op.endswith("_lse"):
        out, lse = res
    elif op == "attention_bshd_split":
        assert res[0].is_contiguous() and res[1].is_contiguous(), what
        assert res[0].shape[1] == SPLIT, what
        out = torch.cat(list(res), 1)
    else:
        out = res
    if not op.startswith("attention_bshd"):
        out = out.permute(0, 2, 1, 3)
        lse = None if lse is None else lse.permute(0, 2, 1)
    assert out.shape == (B, SQ, H, D) and out.dtype == dtype, what
    if native:
        assert torch.equal(out, want), (
            f"{what}: {(out != want).sum().item()} of {out.numel()} values "
            f"differ from attention_bshd")
    else:
        C.check(out, want, what=what)
    if lse is not None:
        # the pad route slices the output only
        assert lse.shape == (B, SQ, H) and lse.dtype == torch.float32, what
        C.check(lse, _reference(D, dtype, mask)[1], what=what + " lse")


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize("op,mask", CELLS, ids=[f"{o}-{m}" for o, m in CELLS])
def test_route(op, mask, dtype, D, spy):
    """The bindings reached, the head dim they received, the notes given,
    and the output: the bits of attention_bshd on the same data (of the
    zero-padded call for attention_bshd itself) wherever a kernel ran, the
    fp32 reference within the suite's tolerance where none did."""
    _check_route(op, mask, D, dtype, spy)


@pytest.mark.parametrize("op", list(BINDING))
def test_fp32_reaches_no_binding(op, spy):
    """fp32 has no native instantiation: no binding, the op's own note (and
    attention_bshd's for the split op, which composes it)."""
    assert (BINDING[op], "dtype=torch.float32, D=64") in expected(
        op, "none", 64, torch.float32)[1]
    _check_route(op, "none", 64, torch.float32, spy)
