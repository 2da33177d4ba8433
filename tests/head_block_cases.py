"""Inputs of the per-head block-mask and top-p selector tests (CPU tensors).

Selector inputs: every query row of block qb of (b, h) is a[qb] * u, every key
row of tile t is (l[t] / sqrt(D)) * u, u a +-1 vector of (b, h), plus N(0,
NOISE^2) noise, so the pooled score of tile t is a[qb] * l[t] to about 1e-3.
l is a ladder, -step * rank, scattered over the tiles by a permutation that
differs per (b, h); two tiles share one rank and hold bit-identical K rows.
Step and tie rank are chosen, from the masses exp(-step * rank) / sum, so
that at top_p = 0.5 and 0.9 the kept mass clears top_p by 0.008 or more on
both sides and the tie pair straddles 0.5 (one of the pair would reach it).
test_head_block_mask_reference.py asserts the margins on the fp64 reference.
"""
import functools
import math

import torch

from comfyui_parallelanything_amd.ops import reference as R

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SQ, SK = 600, 321       # 3 query blocks (the last 88 rows), 6 tiles (1 key)
TOP_PS = (0.5, 0.9, 1.0)
NOISE = 0.004
Q_GAINS = (1.0, 0.9, 1.05)   # a[qb]
# name: B, H, Sq, Sk, ladder step, rank of the tie pair, with a keep mask;
# big is 300 tiles, a second trip of every per-thread tile loop
SELECT_CASES = {"small": (2, 2, SQ, SK, -math.log(0.6), 1, False),
                "big": (1, 2, 256, 19200, 0.178, 4, True)}


@functools.lru_cache(maxsize=None)
def select_case(name, D, dt):
    """dict(q, k [B, H, S, D] in dtype, keep [nq, nk] or None)."""
    B, H, Sq, Sk, step, tie, with_keep = SELECT_CASES[name]
    nq, nk = R.block_mask_shape(Sq, Sk)
    g = torch.Generator(device="cpu").manual_seed(7 * D + nk)
    u = (torch.randint(0, 2, (B, H, 1, D), generator=g) * 2 - 1).float()
    # ranks 0 .. tie, tie, tie + 1, ...: nk entries, one rank twice
    ranks = torch.tensor([r - (r > tie) for r in range(nk)]).float()
    gain = torch.tensor(Q_GAINS)[torch.arange(Sq) // R.Q_BLOCK]
    q = (gain[:, None] * u).contiguous()
    k = torch.empty(B, H, Sk, D)
    # tile t of (b, h) sits at ladder position pos[b, h, t]; the shift keeps
    # the tie pair off the partial last tile
    pos = (torch.arange(nk) * 7 + 4 + 2 * torch.arange(B)[:, None, None]
           + torch.arange(H)[None, :, None]) % nk
    ladder = (-step * ranks[pos]).repeat_interleave(R.KV_TILE, -1)[..., :Sk]
    k = ladder[..., None] / math.sqrt(D) * u
    q = q + NOISE * torch.randn(q.shape, generator=g)
    k = (k + NOISE * torch.randn(k.shape, generator=g)).to(DTYPES[dt])
    for b in range(B):
        for h in range(H):
            t0 = (pos[b, h] == tie).nonzero().item()
            t1 = (pos[b, h] == tie + 1).nonzero().item()
            k[b, h, 64 * t1:64 * t1 + 64] = k[b, h, 64 * t0:64 * t0 + 64]
    keep = torch.rand(nq, nk, generator=g) < 0.05 if with_keep else None
    return dict(q=q.to(DTYPES[dt]), k=k, keep=keep)


@functools.lru_cache(maxsize=None)
def select_ref(name, D, dt, top_p):
    """The fp64 reference's mask of a case, bool [B, H, nq, nk]."""
    c = select_case(name, D, dt)
    return R.select_block_mask(c["q"], c["k"], top_p, keep=c["keep"])


def head_mask(B, H, Sq=SQ, Sk=SK):
    """Per-head block mask [B, H, nq, nk], different for every (b, h): tile t
    live for query block qb iff (t + qb + h + 2 b) % 3 != 0, but tile (b + h)
    % nk, which no query block of (b, h) visits; (b, h, qb) = (B - 1, H - 1,
    nq - 1) has no live tile."""
    nq, nk = R.block_mask_shape(Sq, Sk)
    b, h, qb, t = torch.meshgrid(torch.arange(B), torch.arange(H),
                                 torch.arange(nq), torch.arange(nk),
                                 indexing="ij")
    m = ((t + qb + h + 2 * b) % 3 != 0) & (t != (b + h) % nk)
    m[B - 1, H - 1, nq - 1] = False
    return m


def key_mask(B, Sk=SK):
    """[B, Sk] all true but tile 1 of the last batch element."""
    keys = torch.ones(B, Sk, dtype=torch.bool)
    keys[B - 1, 64:128] = False
    return keys


def seen_keys(mask, keys, Sk=SK):
    """[B, H, Sk]: keys some query block of (b, h) sees."""
    return mask.any(2).repeat_interleave(64, -1)[..., :Sk] & keys[:, None]
