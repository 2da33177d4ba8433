"""Dense-mask patterns of test_attn_bits_reference.py and test_gpu_attn_bits.py:
B=2, H=2, Sq=300 (one full query block and one of 44 rows), Sk=200 (three
full tiles and an 8-key tail), negative_scores inputs. CPU-only, deterministic."""
import functools

import torch

import kernel_cases as C

B, H, SQ, SK = 2, 2, 300, 200
EMPTY = (7, 255, 256, 299)              # bernoulli rows that see nothing
DEAD_KEYS = slice(130, 141)             # dontcare: seen by nobody, K/V = NaN
_I, _J = torch.arange(SQ)[:, None], torch.arange(SK)[None, :]


# rows < 100 see keys [0, 70), the others [70, 200): tile 0 is full for some
# rows of block 0 and dead for the others, which meet it first; block 1 skips
# it; tile 2 is full for block 1; the tail is partial for both
_REGIONS = ((_I < 100) & (_J < 70)) | ((_I >= 100) & (_J >= 70))
PATTERNS = {"bernoulli": torch.rand(B, SQ, SK, generator=C._gen(77)) < 0.5,
            "regions": _REGIONS, "dontcare": _REGIONS.clone()}
PATTERNS["bernoulli"][:, EMPTY] = False
PATTERNS["dontcare"][:, DEAD_KEYS] = False


def dense(mask):
    """[B, SQ, SK] whatever the pattern's own rank."""
    return mask.expand(B, SQ, SK)


@functools.lru_cache(maxsize=None)
def qkv(D, dtype, Sk=SK):
    return C.negative_scores(B, H, SQ, Sk, D, dtype, 7000 + D)


def poisoned(k, v):
    """k, v with NaN at DEAD_KEYS."""
    k, v = k.clone(), v.clone()
    k[:, :, DEAD_KEYS] = float("nan")
    v[:, :, DEAD_KEYS] = float("nan")
    return k, v
