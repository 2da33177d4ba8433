"""Inputs off N(0,1) for the kernel numerics tests, and plain-torch
emulations of the kernels' arithmetic that take a ``fault=``.

Shared by test_kernel_cases_reference.py (CPU: proves that these inputs and
criteria reject a subtly wrong kernel), test_gpu_attn_regimes.py and
test_gpu_norm_regimes.py (GPU: run the real kernels on them). Everything
here is CPU-only and deterministic; the GPU tests move the tensors over.

Why not randn: with N(0,1) scores a key that wrongly enters the softmax with
score 0 and V = 0 weighs about 1/Sk, far below rtol = atol = 2e-2; and the
mean of a randn row is about 0, its variance about 1, so a LayerNorm that
skipped the mean or ignored eps passes too.
"""
import math

import torch

from comfyui_parallelanything_amd.ops import reference as R

BF16 = torch.bfloat16
F16 = torch.float16
DTYPES = (BF16, F16)
DTYPE_IDS = ("bf16", "fp16")
DIMS = (64, 128)
RTOL = ATOL = 2e-2           # every attention comparison in this project
KV = R.KV_TILE               # 64 keys per tile
QB = R.Q_BLOCK               # 256 query rows per block


def passes(out, ref, rtol=RTOL, atol=ATOL):
    """The one comparison of all three files: torch.testing.assert_close on
    fp32 CPU copies, NaN never equal. True / False instead of raising."""
    try:
        check(out, ref, rtol, atol)
    except AssertionError:
        return False
    return True


def check(out, ref, rtol=RTOL, atol=ATOL, what="", equal_nan=False):
    """Against an fp32 or fp64 reference: compared in the reference's type,
    so an fp64 reference is not rounded first."""
    ref = ref.cpu()
    if ref.dtype != torch.float64:
        ref = ref.float()
    torch.testing.assert_close(
        out.cpu().to(ref.dtype), ref, rtol=rtol, atol=atol,
        equal_nan=equal_nan,
        msg=(lambda m: f"{what}: {m}") if what else None)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# --------------------------------------------------------------------------
# Attention inputs: (B, H, Sq, Sk, D, dtype, seed) -> q [B,H,Sq,D], k, v
# [B,H,Sk,D] on the CPU, already rounded to dtype.
# --------------------------------------------------------------------------

def negative_scores(B, H, Sq, Sk, D, dtype, seed):
    """Every real key's scaled score is about -6 (measured over every case
    here: -13.3 .. -1.1), so a phantom key with score 0 takes a quarter of
    the softmax or more instead of 1/Sk. The sum of exp(score) over the keys
    grows with their number, so beyond 128 keys they sink by ln(Sk / 128): -6.4
    at Sk = 193, -6.9 at 320 (with a flat -6 one row in 800 of the Sk = 320
    key-mask cases fell to w = 0.21)."""
    g = _gen(seed)
    depth = 6.0 + math.log(max(Sk, 128) / 128)
    u = torch.randn(B, H, 1, D, generator=g)
    u = u * (math.sqrt(D) / u.norm(dim=-1, keepdim=True))
    q = u + 0.5 * torch.randn(B, H, Sq, D, generator=g)
    k = -(depth / math.sqrt(D)) * u + torch.randn(B, H, Sk, D, generator=g)
    v = torch.randn(B, H, Sk, D, generator=g)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def uniform_ones(B, H, Sq, Sk, D, dtype, seed):
    """q = 0, v = 1: the output is exactly 1.0 where a row sees a key (every
    weight is 1/n and they sum to 1 whatever their rounding, as long as no
    zero-V phantom takes part) and exactly 0 where it sees none."""
    g = _gen(seed)
    q = torch.zeros(B, H, Sq, D)
    k = torch.randn(B, H, Sk, D, generator=g)
    v = torch.ones(B, H, Sk, D)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def staircase(B, H, Sq, Sk, D, dtype, seed, reverse=False):
    """randn with the K rows of tile t scaled by 1 + t: the running maximum
    grows on (almost) every tile, so the alpha rescale of the accumulators
    runs each time. reverse=True scales by n_tiles - t: after tile 0 the
    maximum (almost) never grows, alpha is exactly 1 and the rescale is
    skipped."""
    g = _gen(seed)
    q = torch.randn(B, H, Sq, D, generator=g)
    k = torch.randn(B, H, Sk, D, generator=g)
    v = torch.randn(B, H, Sk, D, generator=g)
    nt = (Sk + KV - 1) // KV
    t = torch.arange(Sk) // KV
    step = (nt - t) if reverse else (1 + t)
    k = k * step[None, None, :, None].float()
    return q.to(dtype), k.to(dtype), v.to(dtype)


ATTN_BUILDERS = {"negative_scores": negative_scores,
                 "uniform_ones": uniform_ones}

# ---- key masks [Sk] (CPU bool); patterns of test_gpu_attn_mask.py ---------


def bernoulli(sk):
    return torch.rand(sk, generator=_gen(sk)) < 0.5


def hole(sk):
    a = torch.arange(sk)
    return ~((a >= 30) & (a < max(sk - 30, 34)))


def one_in_last_tile(sk):
    m = torch.zeros(sk, dtype=torch.bool)
    m[sk - 1] = True
    if sk > KV:
        m[:10] = True
    return m


def walking_dead(sk, start=0, stride=13):
    """All live but one key per tile, at bit (start + stride * t) % 64 of
    tile t (skipped where that lies beyond Sk): the partial tiles closest to
    full, one constant bit position of the substitution each."""
    m = torch.ones(sk, dtype=torch.bool)
    for t in range((sk + KV - 1) // KV):
        j = KV * t + (start + stride * t) % KV
        if j < sk:
            m[j] = False
    return m


def key_mask_stack(sk):
    """[5, Sk]: bernoulli, hole, one-in-last-tile, walking dead key, and an
    empty batch element (zeros for it, by contract)."""
    return torch.stack([bernoulli(sk), hole(sk), one_in_last_tile(sk),
                        walking_dead(sk), torch.zeros(sk, dtype=torch.bool)])


# ---- the cases the GPU tests run (the CPU test walks the same lists) ------

TAIL_SK = (1, 63, 65, 193)
TAIL_SQ = (40, 300)
CONTROL_SK = 128             # every tile full
OVERREAD_SK = (1, 65, 193)
MASK_SK = (100, 193, 320)
MASK_SQ = 300
BLOCK_SQ, BLOCK_SK = 600, 321
STAIR_SQ, STAIR_SK = 300, 320
PAD_DIMS = (40, 80)          # zero-padded to 64 / 128 by attention_bshd
PAD_SK = 100                 # (at D=40, Sk=193 one row in 2500 has w = 0.23)


def tail_case(regime, D, dtype, Sq, Sk):
    """Unmasked, B=1, H=2."""
    q, k, v = ATTN_BUILDERS[regime](1, 2, Sq, Sk, D, dtype, 1000 + Sk)
    return dict(q=q, k=k, v=v, keys=None, block=None)


def mask_case(regime, D, dtype, Sk, Sq=MASK_SQ):
    keys = key_mask_stack(Sk)
    q, k, v = ATTN_BUILDERS[regime](keys.shape[0], 2, Sq, Sk, D, dtype,
                                    2000 + Sk)
    return dict(q=q, k=k, v=v, keys=keys, block=None)


def block_case(regime, D, dtype, key_seeds=(80, 81)):
    """Query block 0 attends tiles 0, 2, 3, 5, block 1 tiles 1, 2, 5, block 2
    (rows 512..599) none, composed with Bernoulli(0.5) keys per batch
    element: live lists of different lengths, and rows that see nothing.
    B*H = 8 takes the XCD-affine grid."""
    Sq, Sk = BLOCK_SQ, BLOCK_SK
    nq, nk = R.block_mask_shape(Sq, Sk)
    block = torch.zeros(nq, nk, dtype=torch.bool)
    block[0, [0, 2, 3, 5]] = True
    block[1, [1, 2, 5]] = True
    keys = torch.stack([torch.rand(Sk, generator=_gen(s)) < 0.5
                        for s in key_seeds])
    q, k, v = ATTN_BUILDERS[regime](2, 4, Sq, Sk, D, dtype, 3000)
    return dict(q=q, k=k, v=v, keys=keys, block=block)


def staircase_case(D, dtype, reverse, masked):
    q, k, v = staircase(1, 2, STAIR_SQ, STAIR_SK, D, dtype, 4000, reverse)
    keys = torch.ones(1, STAIR_SK, dtype=torch.bool) if masked else None
    return dict(q=q, k=k, v=v, keys=keys, block=None)


def attn_ref(case, scale=None):
    """fp32 reference of a case, [B, H, Sq, D]."""
    return R.attention(case["q"].float(), case["k"].float(),
                       case["v"].float(), scale, key_mask=case["keys"],
                       block_mask=case["block"])


def visibility(case):
    """bool [B, Sq, Sk]: key j visible to query row i of batch element b."""
    B, _, Sq, _ = case["q"].shape
    Sk = case["k"].shape[2]
    vis = torch.ones(B, Sq, Sk, dtype=torch.bool)
    if case["block"] is not None:
        vis &= case["block"].repeat_interleave(QB, 0).repeat_interleave(
            KV, 1)[None, :Sq, :Sk]
    if case["keys"] is not None:
        vis &= case["keys"][:, None, :]
    return vis


def phantom_weight(case, scale=None):
    """w [B, H, Sq] = 1 / (1 + sum over visible keys of exp(score)): the
    softmax weight one extra key with score 0 would take."""
    q, k = case["q"].double(), case["k"].double()
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    s = s.masked_fill(~visibility(case)[:, None], float("-inf"))
    return 1.0 / (1.0 + torch.exp(s).sum(-1))


def processed_tiles(case):
    """[(b, query block, tile, live bits [64])] of every tile the kernel
    processes; the bits are the tile's mask word (False at and beyond Sk)."""
    B, _, Sq, _ = case["q"].shape
    Sk = case["k"].shape[2]
    nq, nk = R.block_mask_shape(Sq, Sk)
    keys = case["keys"]
    masked = keys is not None or case["block"] is not None
    if keys is None:
        keys = torch.ones(B, Sk, dtype=torch.bool)
    words = torch.zeros(B, nk * KV, dtype=torch.bool)
    words[:, :Sk] = keys
    words = words.view(B, nk, KV)
    out = []
    for b in range(B):
        for qb in range(nq):
            for t in range(nk):
                if masked and not words[b, t].any():
                    continue                    # dead tile: never processed
                if case["block"] is not None and not case["block"][qb, t]:
                    continue
                out.append((b, qb, t, words[b, t]))
    return out


# --------------------------------------------------------------------------
# Emulation of attn_fwd_v4_kernel's tile loop (ops/hip/attention.h): 64-key
# tiles, dead K/V rows staged as zeros, -3e30 substituted for dead keys of a
# partial tile, -1e30 initial running maximum, raw-score maximum scaled
# afterwards, exp2 with the scale folded in, P rounded to the element type
# before P.V, fp32 accumulators, alpha rescale skipped when alpha == 1.
#
# fault: None, or one of
#   ("sentinel", r)   the substitution misses bit position r of partial tiles
#   ("tail", +1|-1)   unmasked validity test key < Sk + d (staging stays right)
#   ("full",)         every processed tile takes the `full` branch
#   ("alpha", j)      the accumulators miss the rescale on the j-th tile
# --------------------------------------------------------------------------

ATTN_FAULTS = ([("sentinel", r) for r in range(KV)]
               + [("tail", 1), ("tail", -1), ("full",), ("alpha", 1)])


def emulate_attention(case, scale=None, fault=None):
    q, k, v = case["q"], case["k"], case["v"]
    dtype = q.dtype
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    scale2 = torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    nq, nk = R.block_mask_shape(Sq, Sk)
    masked = case["keys"] is not None or case["block"] is not None
    kind = fault[0] if fault else None

    kf = torch.zeros(B, H, nk * KV, D)
    vf = torch.zeros(B, H, nk * KV, D)
    kf[:, :, :Sk] = k.float()
    vf[:, :, :Sk] = v.float()
    qf = q.float()
    out = torch.zeros(B, H, Sq, D)
    tiles = {}
    for b, qb, t, bits in processed_tiles(case):
        tiles.setdefault((b, qb), []).append((t, bits))
    for b in range(B):
        for qb in range(nq):
            r0, r1 = qb * QB, min(qb * QB + QB, Sq)
            n = r1 - r0
            m_run = torch.full((H, n), -1e30)
            l_run = torch.zeros(H, n)
            o = torch.zeros(H, n, D)
            for j, (t, bits) in enumerate(tiles.get((b, qb), [])):
                stage = bits.clone()            # issue_tile_loads: its own
                valid = bits.clone()            # softmax_phase
                if kind == "tail" and not masked:
                    valid = torch.arange(KV) + t * KV < Sk + fault[1]
                full = bool(valid.all())
                if kind == "full":
                    full = True
                if kind == "sentinel" and not full:
                    valid[fault[1]] = True
                kt = kf[b, :, t * KV:(t + 1) * KV] * stage[None, :, None]
                vt = vf[b, :, t * KV:(t + 1) * KV] * stage[None, :, None]
                st = torch.matmul(qf[b, :, r0:r1], kt.transpose(-1, -2))
                if not full:
                    st = torch.where(valid[None, None, :], st,
                                     torch.tensor(-3e30))
                mx = st.amax(-1)
                mnew = torch.maximum(m_run, mx * scale2)
                alpha = torch.exp2(m_run - mnew)
                m_run = mnew
                p = torch.exp2(st * scale2 - mnew[..., None])
                l_run = l_run * alpha + p.sum(-1)
                if not (kind == "alpha" and j == fault[1]):
                    o = o * alpha[..., None]
                o = o + torch.matmul(p.to(dtype).float(), vt)
            inv = torch.where(l_run > 0, 1.0 / l_run, torch.zeros(()))
            out[b, :, r0:r1] = o * inv[..., None]
    return out.to(dtype)


# --------------------------------------------------------------------------
# Norm rows: (rows, D, dtype, seed) -> [rows, D] on the CPU, rounded to dtype
# --------------------------------------------------------------------------

def plain(rows, D, dtype, seed):
    return torch.randn(rows, D, generator=_gen(seed)).to(dtype)


def tiny(rows, D, dtype, seed):
    """Variance about 1e-6: as large as the default eps."""
    return (1e-3 * torch.randn(rows, D, generator=_gen(seed))).to(dtype)


def offset(rows, D, dtype, seed):
    """Mean 40, variance 1: E[x^2] - mean^2 cancels three digits, and a
    skipped mean subtraction is 40 sigma."""
    return (40.0 + torch.randn(rows, D, generator=_gen(seed))).to(dtype)


def outlier(rows, D, dtype, seed):
    """One 500 per row, at index 0, D-1 or D/2+3 by turns: another lane and
    wave of the reduction each."""
    x = torch.randn(rows, D, generator=_gen(seed))
    pos = (0, D - 1, min(D // 2 + 3, D - 1))
    for r in range(rows):
        x[r, pos[r % 3]] = 500.0
    return x.to(dtype)


CONSTANTS = (77.7, 333.3, 9.87, 19.99, 2047.0, 60000.0, 1001.0, 1.0,
             0.1, 3.14159, 0.007, 40.0, 100.0, 513.0, 5000.0, 12345.0)
CONSTANT_ROWS = 2 * len(CONSTANTS)


def constant(rows, D, dtype, seed=0):
    """Row i is constant: CONSTANTS[i % 16], negated for the second sixteen
    (row i of CONSTANT_ROWS rows holds constant_value(i))."""
    c = torch.tensor([constant_value(i) for i in range(rows)])
    return c[:, None].expand(rows, D).to(dtype).contiguous()


def constant_value(i):
    c = CONSTANTS[i % len(CONSTANTS)]
    return -c if (i // len(CONSTANTS)) % 2 else c


def huge(rows, D, dtype, seed):
    """+-3e4 (fp16) or +-1e15 (bf16, fp32), signs at random: D * x^2 stays
    below 1e38 for every D used here, so fp32 sums must not overflow."""
    mag = 3e4 if dtype == F16 else 1e15
    sign = torch.randint(0, 2, (rows, D), generator=_gen(seed)) * 2 - 1
    return (mag * sign.float()).to(dtype)


NORM_REGIMES = {"tiny": tiny, "offset": offset, "outlier": outlier,
                "constant": constant, "huge": huge}


def norm_rows(regime, rows, D, dtype, seed=0):
    fn = plain if regime == "plain" else NORM_REGIMES[regime]
    return fn(rows, D, dtype, seed)


# Per-op (rtol, atol) of test_gpu_kernels.py
TOL_RMS = (2e-2, 2e-2)
TOL_LN = (2e-2, 5e-2)
TOL_GN = (2e-2, 5e-2)
TOL_QK = (3e-2, 3e-2)
TOL_GELU = (2e-2, 2e-2)
TOL_FP32 = (1e-5, 1e-5)

# Constant rows on which only finiteness is asserted, per op: those where
# the fp32 two-pass reference (F.layer_norm / F.group_norm on the CPU, as
# ops.reference calls them, with the affine of the test) is itself more than
# a quarter of the tolerance from fp64 at some shape and dtype used here.
# (x - mean) * rsqrt(var + eps) of a constant row is ill-conditioned at large
# magnitude: a rounding delta of the mean, or of x * s - mean * s where the
# affine is folded in as F.group_norm does, comes out times rsqrt(eps) =
# 1000. LayerNorm has none: the mean of D <= 8192 equal 16-bit values is
# exact in fp32 (n * c fits 24 bits), so x - mean is exactly 0.
# test_kernel_cases_reference.py checks both lists.
FINITE_ONLY_CONSTANTS = {
    "rms_norm": (),                  # no cancellation: c * rsqrt(c * c + eps)
    "layer_norm_mod": (),
    "group_norm_silu": (513.0, 1001.0, 2047.0, 5000.0, 12345.0, 60000.0),
}
# fp32 inputs, held to 1e-5: F.layer_norm is close on all sixteen, but
# F.group_norm's folded affine leaves only these within 2.5e-6 of fp64, so
# on fp32 GroupNorm the other fourteen are checked for finiteness only
FP32_GROUP_NORM_COMPARED = (0.1, 0.007)


def compared_constant(op, dtype, i):
    """Row i of constant() is compared for closeness, not only finiteness."""
    c = CONSTANTS[i % len(CONSTANTS)]
    if dtype == torch.float32 and op == "group_norm_silu":
        return c in FP32_GROUP_NORM_COMPARED
    return c not in FINITE_ONLY_CONSTANTS[op]


# (regime, eps) every norm op runs: each regime at the default eps, and randn
# and tiny rows with eps passed as 1e-2 and 1e-5 (on randn alone an ignored
# eps = 1e-2 moves the output by 0.5%, inside the tolerance; on tiny rows it
# is a factor of 100)
EPS_VALUES = (1e-2, 1e-5)
NORM_RUNS = tuple((r, 1e-6) for r in (
    "tiny", "offset", "outlier", "constant", "huge")) + tuple(
    (r, e) for e in EPS_VALUES for r in ("plain", "tiny"))


def norm_tol(dtype, tol16):
    return TOL_FP32 if dtype == torch.float32 else tol16


RMS_SHAPES = ((5, 128), (5, 512), (5, 8), (5, 2056), (5, 5120), (5, 20))
LN_DIMS = (8, 64, 2056, 3072, 5120, 20)     # 20: the scalar kernel
GN_SHAPES = ((1, 8, 3, 3, 4), (2, 32, 5, 7, 4), (1, 8, 4, 4, 8))
QK_DIMS = (40, 128)


def rms_norm_f64(x, w=None, eps=1e-6):
    xd = x.double()
    out = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
    return out if w is None else out * w.double()


def layer_norm_f64(x, eps=1e-6):
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = (xd - mean).pow(2).mean(-1, keepdim=True)
    return (xd - mean) * torch.rsqrt(var + eps)


def layer_norm_mod_f64(x, scale, shift, eps=1e-6):
    """x [B, S, D], scale/shift [B, D]."""
    return (layer_norm_f64(x, eps) * (1.0 + scale.double()[:, None])
            + shift.double()[:, None])


def group_norm_silu_f64(x, groups, w=None, b=None, eps=1e-6):
    B, C = x.shape[:2]
    xd = x.double().reshape(B, groups, -1)
    out = layer_norm_f64(xd, eps).reshape(x.shape)
    if w is not None:
        out = out * w.double()[None, :, None, None] \
            + b.double()[None, :, None, None]
    return out * torch.sigmoid(out)


def rope_f64(x, cs):
    """x [B, S, H, D], cs [S, D/2, 2]: adjacent pairs rotated."""
    B, S, H, D = x.shape
    xd = x.double().reshape(B, S, H, D // 2, 2)
    cos = cs.double()[None, :, None, :, 0]
    sin = cs.double()[None, :, None, :, 1]
    x0, x1 = xd[..., 0], xd[..., 1]
    return torch.stack([x0 * cos - x1 * sin, x0 * sin + x1 * cos],
                       dim=-1).reshape(B, S, H, D)


def qk_norm_rope_f64(x, w, cs, eps=1e-6):
    return rope_f64(rms_norm_f64(x, w, eps), cs)


def modulation(B, D, dtype, seed):
    g = _gen(seed)
    return (torch.randn(B, D, generator=g).to(dtype),
            torch.randn(B, D, generator=g).to(dtype))


def group_norm_case(regime, shape, dtype):
    """(x [B, C, H, W], w [C], b [C], G) with one regime row per group, in
    (b, g) order. Constant rows take CONSTANT_ROWS // G batch elements, so
    group i holds constant_value(i)."""
    B, Cn, H, W, G = shape
    if regime == "constant":
        B = CONSTANT_ROWS // G
    per = (Cn // G) * H * W
    x = norm_rows(regime, B * G, per, dtype, per).reshape(B, Cn, H, W)
    return x, plain(1, Cn, dtype, 7)[0], plain(1, Cn, dtype, 8)[0], G


def gelu_values(dtype):
    """Zeros, the linear and saturated ranges, the largest finite values the
    cubic must survive, infinities and NaN; a multiple of 8 long."""
    vals = [0.0, 1e-4, 3.0, 8.0, 20.0, 100.0, 3e4, float("inf")]
    if dtype == BF16:
        vals.append(1e30)
    x = torch.tensor(vals)
    x = torch.cat([x, -x, torch.tensor([float("nan")])])
    pad = (-len(x)) % 8
    return torch.cat([x, torch.full((pad,), 0.5)]).to(dtype)


# --------------------------------------------------------------------------
# Emulation of the single-pass row statistics (ops/hip/norm.h): 256 threads,
# thread t takes vectors t, t + 256, ... of `vec` elements (8 in the vector
# kernels, 1 in the scalar ones) and adds x and x*x into two fp32 sums in
# element order; a xor-shuffle tree over each 64-lane wave (offsets 32 .. 1),
# then the four wave sums added in order; mean = s1 / D, var = s2 / D -
# mean^2 clamped at 0, rstd = rsqrt(var + eps). fused=True rounds x*x + s2
# once (fma), fused=False twice: the compiler may pick either.
#
# wide=True is ln_row_stats_wide (layer_norm_mod_fp8_kernel): the per-thread
# fp32 sums are added across the block, and the variance taken, in fp64.
#
# fault: None, "no_eps", "eps_outside", "no_mean", "no_clamp", "skip_last"
# --------------------------------------------------------------------------

NORM_FAULTS = ("no_eps", "eps_outside", "no_mean", "no_clamp", "skip_last")


def _block_sum(vals, fused_sq=None, wide=False):
    """vals [rows, nvec, vec] fp32 -> [rows]; vector i belongs to thread
    i % 256. fused_sq: add the squares, with one rounding per add. wide:
    the 256 thread sums added in fp64, returned as fp64."""
    rows, nvec, vec = vals.shape
    passes_ = (nvec + 255) // 256
    pad = passes_ * 256 - nvec
    v = torch.cat([vals, torch.zeros(rows, pad, vec)], 1).view(
        rows, passes_, 256, vec)
    acc = torch.zeros(rows, 256)
    for p in range(passes_):
        for j in range(vec):
            x = v[:, p, :, j]
            if fused_sq is None:
                acc = acc + x
            elif fused_sq:
                acc = (acc.double() + x.double() * x.double()).float()
            else:
                acc = acc + x * x
    if wide:
        return acc.double().sum(1)
    w = acc.view(rows, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, torch.arange(64) ^ off]
    total = torch.zeros(rows)
    for i in range(4):
        total = total + w[:, i, 0]
    return total


def emulate_row_stats(x, eps=1e-6, fault=None, fused=True, vec=8,
                      deviation_pass=False, wide=False):
    """x [rows, D] -> (mean, rstd, corr), fp32 [rows]. deviation_pass: the
    fp32 instantiations of the scalar kernels, which sum d = x - mean and
    d * d in a further pass: corr = E[d] is what the mean missed, var =
    E[d^2] - corr^2, and the output is ((x - mean) - corr) * rstd."""
    rows, D = x.shape
    xf = x.float().view(rows, D // vec, vec)
    if fault == "skip_last":
        xf = xf[:, :-1]
    s1 = _block_sum(xf, wide=wide)
    s2 = _block_sum(xf, fused_sq=fused, wide=wide)
    mean = s1 / D
    var = s2 / D - mean * mean
    if wide:
        mean, var = mean.float(), var.float()
    corr = torch.zeros_like(mean)
    if deviation_pass:
        d = xf - mean[:, None, None]
        corr = _block_sum(d) / D
        var = _block_sum(d, fused_sq=fused) / D - corr * corr
    if fault != "no_clamp":
        var = torch.clamp(var, min=0.0)
    if fault == "no_eps":
        rstd = torch.rsqrt(var)
    elif fault == "eps_outside":
        rstd = torch.rsqrt(var) + eps
    else:
        rstd = torch.rsqrt(var + eps)
    if fault == "no_mean":
        mean = torch.zeros_like(mean)
    return mean, rstd, corr


def emulate_layer_norm(x, eps=1e-6, fault=None, fused=True, vec=8,
                       deviation_pass=False):
    """LayerNorm of [rows, D] with emulate_row_stats, rounded to x.dtype."""
    mean, rstd, corr = emulate_row_stats(x, eps, fault, fused, vec,
                                         deviation_pass)
    return (((x.float() - mean[:, None]) - corr[:, None])
            * rstd[:, None]).to(x.dtype)
