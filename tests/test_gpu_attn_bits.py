"""Dense attention masks (attn_mask=) on the native kernels, against
ops.reference.attention on fp32 CPU copies at the attention tolerance, and bit
for bit against the three mask families they generalise."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_bits_cases as MC
import kernel_cases as C
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)
DIMS = pytest.mark.parametrize("D", C.DIMS)
BSHD = pytest.mark.parametrize("bshd", [False, True], ids=["bhsd", "bshd"])


@pytest.fixture(autouse=True)
def native_only(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.hip_available("attn_fwd_bshd_split_bits"), "dense-mask kernels missing"

    def refuse(op, why):
        raise AssertionError(f"{op} fell back to the reference path: {why}")

    monkeypatch.setattr(ops, "_unsupported", refuse)


@functools.lru_cache(maxsize=None)
def _ref(D, dtype, name):
    q, k, v = (t.float() for t in MC.qkv(D, dtype))
    return R.attention(q, k, v, attn_mask=MC.PATTERNS[name])


def _run(D, dtype, bshd, Sk=MC.SK, poison=False, **kw):
    """[B, H, Sq, D] over Sk keys; bshd runs on permuted views."""
    q, k, v = MC.qkv(D, dtype, Sk)
    if poison:
        k, v = MC.poisoned(k, v)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    kw = {name: x.cuda() if isinstance(x, torch.Tensor)
          else tuple(t.cuda() for t in x) for name, x in kw.items()}
    if not bshd:
        return ops.attention(q, k, v, **kw)
    return ops.attention_bshd(*(t.permute(0, 2, 1, 3) for t in (q, k, v)),
                              **kw).permute(0, 2, 1, 3)


@pytest.mark.parametrize("name", list(MC.PATTERNS))
@BSHD
@DT
@DIMS
def test_patterns(D, dtype, bshd, name):
    mask = MC.PATTERNS[name]
    out = _run(D, dtype, bshd, poison=name == "dontcare", attn_mask=mask)
    assert torch.isfinite(out).all()
    C.check(out, _ref(D, dtype, name), what=name)
    empty = ~MC.dense(mask).any(-1)                     # [B, Sq]
    assert not out.transpose(1, 2)[empty.cuda()].any(), \
        "a row that sees no key is zero"


_KEYS = torch.stack([C.bernoulli(MC.SK), C.hole(MC.SK)])
_CAUSAL = ops.causal_row_bounds(MC.SQ, MC.SK)
TWINS = {   # name: (Sk, the dense mask, the keyword arguments of its twin)
    "all_true_200": (200, torch.ones(MC.SQ, 200, dtype=torch.bool), {}),
    "all_true_256": (256, torch.ones(MC.SQ, 256, dtype=torch.bool), {}),
    "key_mask": (MC.SK, _KEYS[:, None, :].expand(MC.B, MC.SQ, MC.SK),
                 {"key_mask": _KEYS}),
    "causal": (MC.SK, torch.arange(MC.SK)[None] < _CAUSAL[1][:, None],
               {"row_bounds": _CAUSAL}),
    "batch_expanded": (MC.SK, MC.PATTERNS["regions"], {
        "attn_mask": MC.PATTERNS["regions"][None].expand(MC.B, -1, -1)}),
}


@pytest.mark.parametrize("name", list(TWINS))
@BSHD
@DT
@DIMS
def test_bitwise_twins(D, dtype, bshd, name):
    """Each family the dense mask generalises visits the same tiles: same bits."""
    Sk, mask, twin = TWINS[name]
    assert torch.equal(_run(D, dtype, bshd, Sk, attn_mask=mask),
                       _run(D, dtype, bshd, Sk, **twin))


@DT
@DIMS
def test_split_is_the_unsplit_call_sliced(D, dtype):
    q, k, v = (t.cuda().permute(0, 2, 1, 3) for t in MC.qkv(D, dtype))
    am = ops.pack_attn_mask(MC.PATTERNS["bernoulli"].cuda(), MC.B, MC.SQ, MC.SK)
    whole = ops.attention_bshd(q, k, v, attn_mask=am)
    for split in (100, 256):
        a, b = ops.attention_bshd_split(q, k, v, split, attn_mask=am)
        assert torch.equal(a, whole[:, :split]) and torch.equal(b, whole[:, split:])
    C.check(whole.permute(0, 2, 1, 3), _ref(D, dtype, "bernoulli"))


def test_head_dim_40_pads_and_fp32_takes_the_reference_path(monkeypatch):
    mask = MC.PATTERNS["bernoulli"]
    q, k, v = C.negative_scores(MC.B, MC.H, MC.SQ, MC.SK, 40, C.BF16, 7040)
    ref = R.attention(q.float(), k.float(), v.float(), attn_mask=mask)
    out = ops.attention_bshd(*(t.cuda().permute(0, 2, 1, 3) for t in (q, k, v)),
                             attn_mask=mask.cuda())     # a kernel runs
    C.check(out.permute(0, 2, 1, 3), ref)
    notes = []
    monkeypatch.setattr(ops, "_unsupported", lambda op, why: notes.append(op))
    q, k, v = (t.float() for t in MC.qkv(64, C.BF16))
    out = ops.attention(q.cuda(), k.cuda(), v.cuda(), attn_mask=mask.cuda())
    assert notes == ["attn_fwd"]
    C.check(out, _ref(64, C.BF16, "bernoulli"), *C.TOL_FP32)


def test_refusals_leave_the_next_call_right():
    mask = MC.PATTERNS["regions"].cuda()
    q, k, v = (t.cuda() for t in MC.qkv(64, C.BF16))
    qs = q.permute(0, 2, 1, 3)
    ones = functools.partial(torch.ones, dtype=torch.bool, device="cuda")
    am = ops.pack_attn_mask(mask, MC.B, MC.SQ, MC.SK)
    other = ops.pack_attn_mask(ones(MC.SQ, MC.SK + 64), MC.B, MC.SQ, MC.SK + 64)
    rb = tuple(t.cuda() for t in ops.causal_row_bounds(MC.SQ, MC.SK))
    no = "not supported"
    for match, op, args, kw in (
            ("additive", ops.attention, (q, k, v), {"attn_mask": mask.float()}),
            (r"\[Bm, Sq, Sk\]", ops.attention, (q, k, v), {"attn_mask": mask[:-1]}),
            ("head dimension", ops.attention, (q, k, v),
             {"attn_mask": mask.expand(MC.B, 2, -1, -1)}),
            (no, ops.attention, (q, k, v), {"attn_mask": am, "key_mask": ones(MC.B, MC.SK)}),
            (no, ops.attention, (q, k, v), {"attn_mask": am, "block_mask": ones(2, 4)}),
            (no, ops.attention, (q, k, v), {"attn_mask": am, "row_bounds": rb}),
            (no, ops.attention_lse, (q, k, v), {"attn_mask": am}),
            (no, ops.attention_bshd_lse, (qs, qs, qs), {"attn_mask": am}),
            ("packed for", ops.attention, (q, k, v), {"attn_mask": other})):
        with pytest.raises(ValueError, match=match):
            op(*args, **kw)
        C.check(ops.attention(q, k, v, attn_mask=am), _ref(64, C.BF16, "regions"))
