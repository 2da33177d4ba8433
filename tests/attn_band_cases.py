"""Row-bounds patterns of test_attn_band_reference.py and test_gpu_attn_band.py:
B=1, H=2, Sq=300 (two query blocks, the second partial), Sk=200 (three full
tiles and 8 keys), negative_scores inputs. CPU-only, deterministic."""
import functools
import math

import torch

import kernel_cases as C
from comfyui_parallelanything_amd import ops

SQ, SK = 300, 200
_I = torch.arange(SQ)
_ALL = (torch.zeros(SQ, dtype=torch.int64), torch.full((SQ,), SK))


def _where(rows, lo, hi, base=_ALL):
    return (torch.where(rows, lo, base[0]), torch.where(rows, hi, base[1]))


PATTERNS = {
    "causal": ops.causal_row_bounds(SQ, SK),           # rows 0..99 see nothing
    "window": (_I - 40, _I + 41),                      # block 1 beyond Sk
    "window_diag": (_I - 140, _I - 59),   # about the diagonal: t0 > 0 in block 1
    "frame_1_0": ops.frame_span_row_bounds(6, 50, 1, 0),
    "frame_causal": ops.frame_span_row_bounds(6, 50, None, 0),
    "clamped": (_I - 150, 3 * _I - 100),               # below 0 and past Sk
    "empty_rows": _where(_I < 10, 5, 5),
    "empty_block": _where(_I >= 256, 50, 50),
    # rows 0..127 see key 0, rows 128..255 keys 130..199: each half's tiles
    # hold no live key for the other half and are processed all the same.
    # (With -3e30 for dead scores this case still comes out right: the live
    # tile after the dead ones rescales by alpha = 0. What goes wrong then
    # is a row with no key at all in a block that walks tiles, which gets
    # the mean of V: see EMPTY_ROW_PATTERNS.)
    "sentinel": _where((_I >= 128) & (_I < 256), 130, SK,
                       _where(_I < 128, 0, 1)),
}


# patterns with a row that sees nothing in a query block that walks tiles
EMPTY_ROW_PATTERNS = ("causal", "window", "frame_1_0", "clamped", "empty_rows")


def visible(lo, hi, Sk=SK):
    j = torch.arange(Sk)[None, :]
    return (j >= lo[:, None]) & (j < hi[:, None])


@functools.lru_cache(maxsize=None)
def qkv(D, dtype, Sk=SK):
    return C.negative_scores(1, 2, SQ, Sk, D, dtype, 5000 + D)


def dense_softmax_f64(q, k, v, vis, scale=None):
    """fp64 masked softmax on [B, H, S, D]; a row that sees nothing is 0."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return torch.matmul(p, v.double())
