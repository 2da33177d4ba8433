"""Row bounds (row i sees keys lo[i] <= j < hi[i]) on the native kernels, against
ops.reference.attention on fp32 CPU copies at the attention tolerance."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_band_cases as BC
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
    assert ops.hip_available("attn_fwd_bshd_band"), "row-bounds kernels missing"

    def refuse(op, why):
        raise AssertionError(f"{op} fell back to the reference path: {why}")

    monkeypatch.setattr(ops, "_unsupported", refuse)


@functools.lru_cache(maxsize=None)
def _ref(D, dtype, name):
    q, k, v = (t.float() for t in BC.qkv(D, dtype))
    return R.attention(q, k, v, row_bounds=BC.PATTERNS[name])


def _run(D, dtype, bshd, row_bounds=None, Sk=BC.SK, **kw):
    """[B, H, Sq, D] over Sk keys; bshd runs on permuted views."""
    q, k, v = (t.cuda() for t in BC.qkv(D, dtype, Sk))
    if row_bounds is not None and not isinstance(row_bounds, ops.RowBounds):
        row_bounds = tuple(t.cuda() for t in row_bounds)
    if not bshd:
        return ops.attention(q, k, v, row_bounds=row_bounds, **kw)
    return ops.attention_bshd(*(t.permute(0, 2, 1, 3) for t in (q, k, v)),
                              row_bounds=row_bounds, **kw).permute(0, 2, 1, 3)


@pytest.mark.parametrize("name", list(BC.PATTERNS))
@BSHD
@DT
@DIMS
def test_patterns(D, dtype, bshd, name):
    lo, hi = BC.PATTERNS[name]
    out = _run(D, dtype, bshd, (lo, hi))
    C.check(out, _ref(D, dtype, name), what=name)
    empty = lo.clamp(0, BC.SK) >= hi.clamp(0, BC.SK)
    # exact: what catches a -3e30 sentinel (BC.EMPTY_ROW_PATTERNS)
    assert not out[:, :, empty.cuda()].any(), "a row that sees no key is zero"


@pytest.mark.parametrize("Sk", [200, 256, 192])
@BSHD
@DT
@DIMS
def test_bitwise_twins(D, dtype, bshd, Sk):
    """Every key visible is the unmasked call (Sk = 200, 256), bounds on the
    256 / 64 geometry the block_mask= call (Sk = 192): same tiles, same bits."""
    first = torch.arange(BC.SQ) < 256
    lo, hi, kw = torch.where(first, 0, 0), torch.where(first, Sk, Sk), {}
    if Sk == 192:
        lo, hi = torch.where(first, 64, 0), torch.where(first, 192, 128)
        kw = {"block_mask": torch.tensor([[0, 1, 1], [1, 1, 0]]).bool().cuda()}
    assert torch.equal(_run(D, dtype, bshd, (lo, hi), Sk=Sk),
                       _run(D, dtype, bshd, Sk=Sk, **kw))


def test_refusals_leave_the_next_call_right():
    lo, hi = (t.cuda() for t in BC.PATTERNS["causal"])
    q, k, v = (t.cuda() for t in BC.qkv(64, C.BF16))
    qs = q.permute(0, 2, 1, 3)
    ones = functools.partial(torch.ones, dtype=torch.bool, device="cuda")
    rb = ops.pack_row_bounds(lo, hi, BC.SQ, BC.SK)
    other = ops.pack_row_bounds(lo, hi, BC.SQ, BC.SK + 64)
    no = "not supported"
    for match, op, args, kw in (
            ("integer", ops.attention, (q, k, v), {"row_bounds": (lo.float(), hi)}),
            (r"\[300\]", ops.attention, (q, k, v), {"row_bounds": (lo[:-1], hi[:-1])}),
            (no, ops.attention, (q, k, v), {"row_bounds": rb, "key_mask": ones(1, BC.SK)}),
            (no, ops.attention, (q, k, v), {"row_bounds": rb, "block_mask": ones(2, 4)}),
            (no, ops.attention_bshd_split, (qs, qs, qs, 100), {"row_bounds": rb}),
            (no, ops.attention_lse, (q, k, v), {"row_bounds": rb}),
            (no, ops.attention_bshd_lse, (qs, qs, qs), {"row_bounds": rb}),
            ("packed for", ops.attention, (q, k, v), {"row_bounds": other})):
        with pytest.raises(ValueError, match=match):
            op(*args, **kw)
        C.check(ops.attention(q, k, v, row_bounds=rb), _ref(64, C.BF16, "causal"))


def test_pack_and_attention_in_one_graph():
    q, k, v = (t.cuda() for t in BC.qkv(128, C.BF16))
    lo, hi = (t.cuda().clone() for t in BC.PATTERNS["causal"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention(q, k, v, row_bounds=(lo, hi))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = ops.attention(q, k, v, row_bounds=(lo, hi))
    for name in ("sentinel", "window_diag"):
        for dst, src in zip((lo, hi), BC.PATTERNS[name]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out,
                           ops.attention(q, k, v, row_bounds=(lo, hi)))
        C.check(static_out, _ref(128, C.BF16, name), what=name)
