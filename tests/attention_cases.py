"""Attention held to its rounding model: builders, fp64 references, the error
model, the comparison functions and an emulation of attn_fwd_v4_kernel's
arithmetic that takes a ``fault=``.

Shared by test_attention_cases_reference.py (CPU: the faithful emulation
passes every check, every injected arithmetic fault is rejected by a check
the test names) and test_gpu_attn_exact.py (GPU: the native kernels through
the same checks). Masks, tile walk and visibility come from kernel_cases.py.
Everything here is CPU-only and deterministic.

Three kinds of case, docs/KERNELS.md "Attention accuracy contract":
  constant_columns  v[b, h, :, d] = c(b, h, d): the output is c bit for bit
  one_hot_gather    +-1 code words, q = QMUL * k[pi]: one P is exactly 1, all
                    others exactly 0, the output is v[pi] bit for bit
  rounding_model    random data against fp64, by rho = rms(err / sigma) and a
                    rigorous per-element bound
"""
import functools
import math

import torch

import kernel_cases as C
from elementwise_cases import same_bits, spacing16
from comfyui_parallelanything_amd import ops
from comfyui_parallelanything_amd.ops import reference as R

BF16, F16 = C.BF16, C.F16
KV, QB = C.KV, C.QB
SQ, SK = 300, 321            # two query blocks (256 + 32 + 12 rows), five
                             # full tiles and a one-key tail
FUSED_S = 321                # q, k, v of one fused [B, S, 3, H, D] buffer
GRIDS = ((2, 4), (1, 3))     # B*H % 8 == 0: XCD-affine 1-D grid; else 2-D
GRID_IDS = ("xcd", "2d")
LOG2E = 1.4426950408889634

# half the relative spacing of the element type at a power of two: a P
# rounded to nearest is off by at most U of its value
U = {BF16: 2.0 ** -8, F16: 2.0 ** -11}


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int16)


# --------------------------------------------------------------------------
# a. constant_columns
# --------------------------------------------------------------------------

CONSTANTS = (1.0, -1.5, 1.9921875, 2.0 ** -10, 0.3, -7.77, 255.0, 3e4,
             -0.001, 100.0, 17.0)          # 11: a prime, more than B * H
Q_SCALES = (1.0, 3.0)


def column_constants(B, H, D, dtype):
    """c [B, H, D] = CONSTANTS[(d + b * H + h) % 11], rounded to dtype: the
    eleven cyclic shifts are distinct patterns, one per (b, h)."""
    assert B * H <= len(CONSTANTS)
    cs = torch.tensor(CONSTANTS, dtype=torch.float64)
    bh = torch.arange(B * H).view(B, H, 1)
    return cs[(torch.arange(D).view(1, 1, D) + bh) % len(CONSTANTS)].to(dtype)


def constant_columns(B, H, D, dtype, qmul=1.0, Sq=SQ, Sk=SK, mask=None,
                     ones=False):
    """mask: None, "keys" (Bernoulli(0.5) per batch element) or "block"
    (kernel_cases.block_case: Sq = 600, Sk = 321, a block mask composed with
    Bernoulli keys, rows that see nothing). ones=True is uniform_ones'
    construction instead (q = 0, v = 1), kept to show what it cannot see."""
    keys = block = None
    if mask == "block":
        proto = C.block_case("uniform_ones", D, dtype)
        keys, block = proto["keys"], proto["block"]
        B, H, Sq, _ = proto["q"].shape
        Sk = proto["k"].shape[2]
    elif mask == "keys":
        keys = torch.stack([torch.rand(Sk, generator=_gen(90 + b)) < 0.5
                            for b in range(B)])
    g = _gen(5000 + D)
    q = (qmul * torch.randn(B, H, Sq, D, generator=g)).to(dtype)
    k = torch.randn(B, H, Sk, D, generator=g).to(dtype)
    c = column_constants(B, H, D, dtype)
    if ones:
        q, c = torch.zeros_like(q), torch.ones_like(c)
    v = c[:, :, None, :].expand(B, H, Sk, D).contiguous()
    case = dict(q=q, k=k, v=v, keys=keys, block=block)
    seen = C.visibility(case).any(-1)[:, None, :, None]       # [B,1,Sq,1]
    case["want"] = torch.where(seen, c[:, :, None, :],
                               torch.zeros((), dtype=dtype))
    return case


def effective_keys(case, scale=None):
    """1 / sum_j P_j^2 per row, [B, H, Sq] (rows that see no key: inf)."""
    return 1.0 / reference64(case, scale)["P"].pow(2).sum(-1)


def check_constant(out, case, what="constant_columns"):
    """Bit for bit the constants, and +0.0 on a row that sees no key."""
    same_bits(out.cpu(), case["want"], what)


# --------------------------------------------------------------------------
# b. one_hot_gather
# --------------------------------------------------------------------------

# |q| per dim. 64 gives a log2 gap of 346 (D = 64) and 685 (D = 128) between
# the selected key and the next; at D = 40 (the pad route) random code words
# come within 10 of 40 agreeing signs and 64 leaves 146, so q is lengthened.
QMUL = {40: 128.0, 64: 64.0, 80: 64.0, 128: 64.0}
MIN_GAP = 160.0              # > 149: every other exp2 is exactly 0 in fp32
GATHER_VARIANTS = ("rising", "falling", "pair", "dead_twin")
SELECTED_TILE = 1            # the full tile whose 64 positions all get a row


def finite_patterns(dtype):
    """(normal-or-zero-or-subnormal finite bit patterns, as int32 [n]) of a
    16-bit type, and those of them whose magnitude is 2^126 or more (bf16
    only): two of those tied at the maximum of an early tile would overflow
    the fp32 accumulator, and inf * (alpha = 0) is NaN."""
    pat = torch.arange(65536, dtype=torch.int32)
    val = pat.to(torch.int16).view(dtype).float()
    fin = torch.isfinite(val)
    huge = fin & (val.abs() >= 2.0 ** 126)
    return pat[fin & ~huge], pat[huge]


def _rising_keys(Sq, Sk):
    """Sq distinct keys in rising order (needs Sq <= Sk): all of tile
    SELECTED_TILE, the last key, and the rest thinned evenly."""
    assert Sq <= Sk
    must = set(range(SELECTED_TILE * KV, min((SELECTED_TILE + 1) * KV, Sk)))
    must.add(Sk - 1)
    rest = [j for j in range(Sk) if j not in must]
    take = Sq - len(must)
    pick = {rest[(i * len(rest)) // take] for i in range(take)}
    keys = sorted(must | pick)
    assert len(keys) == Sq
    return torch.tensor(keys)


def one_hot_gather(variant, B, H, D, dtype, Sq=SQ, Sk=SK):
    """q [B,H,Sq,D] = QMUL * k[pi]; k +-1 code words; v every finite pattern.

    rising     pi rises with the row: on most rows the maximum arrives in a
               later tile than the first, alpha is exactly 0 there and what
               was accumulated before must vanish
    falling    pi falls: rows of a wave meet their maximum in different
               tiles, and after it alpha is exactly 1
    pair       keys 128..255 repeat the code words of keys 0..127 with other
               V; rows select 0..127; V holds even integers up to 128, so
               the exact output (v1 + v2) / 2 is representable
    dead_twin  Bernoulli key mask (tile 4 the complement of tile 3); pi runs
               over the live keys, and every dead key carries the code word
               of a live one with another V
    """
    g = _gen(7000 + D + GATHER_VARIANTS.index(variant))
    k = (torch.randint(0, 2, (B, H, Sk, D), generator=g) * 2 - 1).float()
    keys = None
    if variant in ("rising", "falling"):
        pi = _rising_keys(Sq, Sk)
        if variant == "falling":
            pi = pi.flip(0)
        pi = pi[None].expand(B, Sq)
    elif variant == "pair":
        k[:, :, 128:256] = k[:, :, 0:128]
        pi = (torch.arange(Sq) % 128)[None].expand(B, Sq)
    else:
        keys = torch.stack([torch.rand(Sk, generator=_gen(95 + b)) < 0.5
                            for b in range(B)])
        # tile 4 the complement of tile 3: between them every position 0..63
        # is live, and selected, in a partial tile
        keys[:, 4 * KV:5 * KV] = ~keys[:, 3 * KV:4 * KV]
        rows = []
        for b in range(B):
            live = keys[b].nonzero().flatten()
            dead = (~keys[b]).nonzero().flatten()
            k[b][:, dead] = k[b][:, live[torch.arange(len(dead)) % len(live)]]
            rows.append(live[(torch.arange(Sq) * len(live)) // Sq])
        pi = torch.stack(rows)
    # V: consecutive finite patterns, a key's row of D in one run; the keys a
    # row selects are numbered first, so the outputs walk the patterns too
    if variant == "pair":
        v = (2 * torch.randint(-64, 65, (B, H, Sk, D), generator=g)).to(dtype)
    else:
        fin, huge = finite_patterns(dtype)
        sel = torch.zeros(Sk, dtype=torch.bool)
        sel[pi[0]] = True
        rank = torch.empty(Sk, dtype=torch.int64)
        rank[torch.cat([sel.nonzero().flatten(),
                        (~sel).nonzero().flatten()])] = torch.arange(Sk)
        slot = ((torch.arange(B * H).view(B, H, 1, 1) * Sk
                 + rank.view(1, 1, Sk, 1)) * D + torch.arange(D))
        vb = fin[slot % len(fin)]
        if len(huge):
            # the last key is in the tile processed last: never accumulated
            # ahead of a row's maximum
            last = torch.arange(B * H * D).view(B, H, D)
            vb[:, :, Sk - 1] = huge[last % len(huge)]
        v = vb.to(torch.int16).view(dtype)
    q = QMUL[D] * torch.gather(
        k, 2, pi[:, None, :, None].expand(B, H, Sq, D))
    case = dict(q=q.to(dtype), k=k.to(dtype), v=v, keys=keys, block=None,
                pi=pi, variant=variant)
    idx = pi[:, None, :, None].expand(B, H, Sq, D)
    want = torch.gather(v, 2, idx)
    if variant == "pair":
        want = ((want.float() + torch.gather(v, 2, idx + 128).float())
                / 2).to(dtype)
    case["want"] = want
    return case


def gather_gap(case):
    """Smallest log2 gap, over all rows, between the selected key's scaled
    score and any other visible key's (a pair's twin excluded), in fp64."""
    q, k = case["q"].double(), case["k"].double()
    B, H, Sq, D = q.shape
    s = torch.matmul(q, k.transpose(-1, -2)) * (LOG2E / math.sqrt(D))
    s = s.masked_fill(~C.visibility(case)[:, None], float("-inf"))
    pi = case["pi"][:, None, :, None].expand(B, H, Sq, 1)
    top = torch.gather(s, 3, pi)
    s = s.scatter(3, pi, float("-inf"))
    if case["variant"] == "pair":
        s = s.scatter(3, pi + 128, float("-inf"))
    return (top - s.amax(-1, keepdim=True)).min().item()


def pattern_classes(want):
    """(normal, zero, subnormal) masks of a 16-bit tensor."""
    f = want.float().abs()
    tiny = 2.0 ** -126 if want.dtype == BF16 else 2.0 ** -14
    return f >= tiny, f == 0, (f > 0) & (f < tiny)


def check_gather(out, case, what="one_hot_gather"):
    """out == v[pi] bit for bit on every normal pattern; a zero comes back
    as a zero of either sign (the accumulator adds +0 products to a -0); a
    subnormal comes back as itself or as a zero. Returns what the subnormals
    and the -0 did: {"subnormal_kept": n, "subnormal_flushed": n,
    "neg_zero_kept": n, "neg_zero_lost": n}."""
    out, want = out.cpu(), case["want"]
    assert out.dtype == want.dtype and out.shape == want.shape, what
    ob, wb = _bits(out).to(torch.int32), _bits(want).to(torch.int32)
    normal, zero, sub = pattern_classes(want)
    bad = normal & (ob != wb)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {int(normal.sum())} normal values "
        f"differ in bits, first at {int(bad.flatten().nonzero()[0])}: "
        f"{out.flatten()[bad.flatten()][0].item()} for "
        f"{want.flatten()[bad.flatten()][0].item()}")
    is_zero = (ob & 0x7fff) == 0
    assert is_zero[zero].all(), f"{what}: a zero of V came back nonzero"
    kept = ob == wb
    assert (kept | is_zero)[sub].all(), (
        f"{what}: a subnormal of V came back as neither itself nor zero")
    negz = zero & (wb != 0)
    return dict(subnormal_kept=int((kept & sub).sum()),
                subnormal_flushed=int((~kept & sub).sum()),
                neg_zero_kept=int((kept & negz).sum()),
                neg_zero_lost=int((~kept & negz).sum()))


# --------------------------------------------------------------------------
# c. rounding_model
# --------------------------------------------------------------------------

MODEL_REGIMES = ("flat_offset", "peaked")
MODEL_SCALES = (None, 0.3)


def rounding_case(regime, B, H, D, dtype, seed=0):
    g = _gen(6000 + 10 * seed + D)
    q = torch.randn(B, H, SQ, D, generator=g)
    k = torch.randn(B, H, SK, D, generator=g)
    v = torch.randn(B, H, SK, D, generator=g)
    if regime == "flat_offset":
        v = 1.0 + 0.1 * v
    else:
        q = 3.0 * q
    return dict(q=q.to(dtype), k=k.to(dtype), v=v.to(dtype), keys=None,
                block=None)


def reference64(case, scale=None):
    """fp64: P [B,H,Sq,Sk] normalised over the visible keys (0 on a row that
    sees none), ref = P v, pav = sum_j P_j |v_j|, p2v2 = sum_j P_j^2 v_j^2,
    sav_l = sum over visible j of |v_j|, over l = sum_j exp(s_j - max s)."""
    q, k, v = (case[n].double() for n in "qkv")
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    vis = C.visibility(case)[:, None]
    s = (torch.matmul(q, k.transpose(-1, -2)) * scale).masked_fill(
        ~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = e.sum(-1, keepdim=True)
    P = e / l.clamp_min(1e-300)
    av = v.abs()
    return dict(P=P, ref=torch.matmul(P, v), pav=torch.matmul(P, av),
                p2v2=torch.matmul(P * P, v * v),
                sav_l=torch.matmul(vis.double().expand_as(P), av)
                / l.clamp_min(1.0))


# The statistic. Model variance of one output: its own rounding (uniform on
# one spacing) plus independent round-to-nearest errors of the P_j, each
# uniform on a width of U * P_j:
#     sigma^2 = spacing(ref)^2 / 12 + U^2 / 12 * sum_j P_j^2 v_j^2
#     rho     = rms((out - ref) / sigma)
# rho of the emulation, five seeds at B, H = 2, 4 and D = 64, 128 (CPU; the
# test recomputes seed 0), in the order flat_offset bf16, flat_offset fp16,
# peaked bf16, peaked fp16:
#     faithful   0.997-1.005  0.998-1.008  0.941-0.957  0.937-0.959
#     trunc      2.05-2.13    2.01-2.12    1.31-1.40    1.30-1.36
#     o16        1.92-2.01    1.91-2.02    1.72-1.75    1.71-1.76
#     scale16    no shift     no shift     1.63-2.60    10.6-19.5
#     qscale16   no shift     no shift     2.60-2.88    2.56-2.82
#     s16        no shift     no shift     6.67-7.46    6.54-7.31
# The limit of a case is the faithful emulation's own rho for that case
# times RHO_MARGIN. The margin covers what the emulation cannot know
# (v_exp_f32 and the reciprocal an ulp either way, the MFMA's accumulation
# order: the CPU file moves the emulation by those and stays below 1.01 of
# its own rho); the nearest fault is trunc on peaked rows at 1.30 / 0.959 =
# 1.36 and on flat rows at 2.0.
RHO_MARGIN = 1.15

# The rigorous per-element bound:
#     |out - ref| <= 0.5 * spacing(ref) + (1 + SLACK) * U * pav  [+ fp16 term]
# A P rounded to nearest is off by at most U * P_j (half a spacing, at the
# bottom of a binade), so with exact arithmetic elsewhere the value ahead of
# the output rounding is within U * pav of fp64. SLACK is what fp32
# arithmetic in the kernel's order adds, in units of U * pav: measured as
# the distance from fp64 of the emulation with P left unrounded
# (emulate(round_p=False, raw=True)), which no rounding decision of a P can
# amplify, over every rounding_model case of this file
# (test_slack_is_twice_the_measured_worst):
#     measured worst   0.0487 of U * pav (fp16, peaked, scale 0.3, D = 128:
#                      U is eight times smaller than in bf16, and the fp32
#                      rounding of scores of size 100 the same; bf16 stays
#                      below 0.007)
#     chosen           SLACK = 2 * 0.0487, rounded up to 0.1
# Twice the worst covers v_exp_f32, the reciprocal and the MFMA's order.
# fp16 term: a P below 2^-14 (relative to the running maximum when it is
# rounded; later rescales only shrink it) is a subnormal of spacing 2^-24,
# off by up to 2^-25 absolutely whatever its size, so key j adds up to
# 2^-25 |v_j| / l.
SLACK_MEASURED = 0.0487
SLACK = 0.1


def model_stats(out, r, dtype, slack=None):
    """(rho, worst |err| / bound) of `out` against reference64's r."""
    slack = SLACK if slack is None else slack
    err = out.cpu().double() - r["ref"]
    sp = spacing16(r["ref"], dtype)
    u = U[dtype]
    sigma2 = sp * sp / 12 + (u * u / 12) * r["p2v2"]
    rho = math.sqrt((err * err / sigma2).mean().item())
    bound = 0.5 * sp + (1 + slack) * u * r["pav"]
    if dtype == F16:
        bound = bound + 2.0 ** -25 * r["sav_l"]
    worst = (err.abs() / bound).max().item()
    return rho, worst


def check_model(out, r, dtype, rho_limit, what="rounding_model"):
    """Both criteria; returns (rho, worst) after printing them."""
    assert out.dtype == dtype and torch.isfinite(out.float()).all(), what
    rho, worst = model_stats(out, r, dtype)
    print(f"{what}: rho {rho:.4f} (limit {rho_limit:.4f}), "
          f"worst |err|/bound {worst:.4f}")
    assert rho <= rho_limit, (
        f"{what}: rho = {rho:.4f} above {rho_limit:.4f} "
        f"({RHO_MARGIN} times the emulation's)")
    assert worst <= 1.0, (
        f"{what}: an element is {worst:.4f} of its rigorous bound from fp64")
    return rho, worst


@functools.lru_cache(maxsize=None)
def model_case(regime, grid, D, dtype, scale):
    """(case, reference64, the emulation's rho), built once, never modified."""
    case = rounding_case(regime, *grid, D, dtype)
    r = reference64(case, scale)
    rho, _ = model_stats(emulate(case, scale), r, dtype)
    return case, r, rho


# --------------------------------------------------------------------------
# Emulation of attn_fwd_v4_kernel's arithmetic (ops/hip/attention.h), as
# kernel_cases.emulate_attention walks it, with the exp2 argument one fused
# multiply-add as the kernel writes it, and arithmetic faults:
#   "trunc"     P converted to 16 bit by truncation (Elem16<E>::pack2)
#   "o16"       the O accumulators rounded to 16 bit once per tile
#   "scale16"   scale2 = scale * log2e rounded to bf16
#   "qscale16"  the scale folded into q, then rounded to the element type
#   "s16"       the QK^T scores rounded to 16 bit ahead of the softmax
#   "l_first"   the running sum l taken from the first tile only
#   "nomax"     the maximum not subtracted
#   "vrot8"     the V rows of a tile rotated by 8 (a tr gather off by a row
#               group)
#   "noxor"     the V image written without the (row & 8) << 1 column XOR
#               that the gather assumes: columns c and c ^ 16 trade on those
#               rows
#   "bhswap"    batch and head swapped in the V pointer
# nudge: +1 / -1 moves every exp2 result and the reciprocal one fp32 ulp up
# or down; flip: P.V summed over the keys of a tile in reverse order. Both
# stand for what the emulation cannot know of the hardware.
# raw=True returns the fp32 values ahead of the output rounding, and
# round_p=False leaves P in fp32 (the SLACK measurement).
# --------------------------------------------------------------------------

ARITH_FAULTS = ("trunc", "o16", "scale16", "qscale16", "s16", "l_first",
                "nomax", "vrot8", "noxor", "bhswap")


def _round_p(p, dtype, trunc):
    if not trunc:
        return p.to(dtype).float()
    if dtype == BF16:
        return (p.view(torch.int32) & -65536).view(torch.float32)
    h = p.to(F16)
    down = (h.float() > p).to(torch.int16)          # p >= 0: one pattern down
    return (h.view(torch.int16) - down).view(F16).float()


def _nudge(x, n):
    if n == 0:
        return x
    to = torch.full_like(x, float("inf") if n > 0 else float("-inf"))
    return torch.where(x > 0, torch.nextafter(x, to), x)


def emulate(case, scale=None, fault=None, nudge=0, flip=False, raw=False,
            round_p=True):
    q, k, v = case["q"], case["k"], case["v"]
    dtype = q.dtype
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    scale2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(
        LOG2E, dtype=torch.float32)
    if fault == "scale16":
        scale2 = scale2.to(BF16).float()
    nq, nk = R.block_mask_shape(Sq, Sk)
    kf = torch.zeros(B, H, nk * KV, D)
    vf = torch.zeros(B, H, nk * KV, D)
    kf[:, :, :Sk] = k.float()
    vf[:, :, :Sk] = v.float()
    if fault == "bhswap":
        bb, hh = torch.arange(B)[:, None], torch.arange(H)[None, :]
        vf = vf[hh % B, bb % H]
    qf = q.float()
    if fault == "qscale16":
        qf = (qf * scale2).to(dtype).float()
        scale2 = torch.ones(())
    xor_rows = ((torch.arange(KV) & 8) != 0)[None, :, None]
    xor_cols = torch.arange(D) ^ 16
    out = torch.zeros(B, H, Sq, D)
    tiles = {}
    for b, qb, t, bits in C.processed_tiles(case):
        tiles.setdefault((b, qb), []).append((t, bits))
    for b in range(B):
        for qb in range(nq):
            r0, r1 = qb * QB, min(qb * QB + QB, Sq)
            n = r1 - r0
            m_run = torch.full((H, n), -1e30)
            l_run = torch.zeros(H, n)
            o = torch.zeros(H, n, D)
            for j, (t, bits) in enumerate(tiles.get((b, qb), [])):
                kt = kf[b, :, t * KV:(t + 1) * KV] * bits[None, :, None]
                vt = vf[b, :, t * KV:(t + 1) * KV] * bits[None, :, None]
                if fault == "vrot8":
                    vt = torch.roll(vt, 8, dims=1)
                if fault == "noxor":
                    vt = torch.where(xor_rows, vt[:, :, xor_cols], vt)
                st = torch.matmul(qf[b, :, r0:r1], kt.transpose(-1, -2))
                if fault == "s16":
                    st = st.to(dtype).float()
                if not bool(bits.all()):
                    st = torch.where(bits[None, None, :], st,
                                     torch.tensor(-3e30))
                mnew = torch.maximum(m_run, st.amax(-1) * scale2)
                if fault == "nomax":
                    mnew = torch.zeros_like(mnew)
                alpha = _nudge(torch.exp2(m_run - mnew), nudge)
                m_run = mnew
                arg = (st.double() * scale2.double()
                       - mnew[..., None].double()).float()      # one fma
                p = _nudge(torch.exp2(arg), nudge)
                ps = p.sum(-1)
                if fault == "l_first" and j > 0:
                    ps = torch.zeros_like(ps)
                l_run = l_run * alpha + ps
                o = o * alpha[..., None]
                p16 = _round_p(p, dtype, fault == "trunc") if round_p else p
                if flip:
                    o = o + torch.matmul(p16.flip(-1), vt.flip(1))
                else:
                    o = o + torch.matmul(p16, vt)
                if fault == "o16":
                    o = o.to(dtype).float()
            inv = torch.where(l_run > 0, _nudge(1.0 / l_run, nudge),
                              torch.zeros(()))
            out[b, :, r0:r1] = o * inv[..., None]
    return out if raw else out.to(dtype)


# --------------------------------------------------------------------------
# A case through ops.attention* on `device` ("cpu": the reference path).
# --------------------------------------------------------------------------

ROUTES = ("bhsd", "bshd", "fused", "split7", "split256")


def run_ops(case, route="bhsd", device="cpu", scale=None):
    """[B, H, Sq, D] out. bhsd: ops.attention. bshd: attention_bshd on
    permuted [B, H, S, D] tensors (strided). fused: attention_bshd on the
    three views of one [B, S, 3, H, D] buffer (needs Sq == Sk). splitN:
    attention_bshd_split at N on permuted tensors, the halves joined."""
    def dev(t):
        return None if t is None else t.to(device)

    q, k, v = (dev(case[n]) for n in "qkv")
    kw = dict(key_mask=dev(case["keys"]), block_mask=dev(case["block"]))
    if route == "bhsd":
        return ops.attention(q, k, v, scale, **kw)
    if route == "fused":
        buf = torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], dim=2)
        q, k, v = buf.unbind(2)
        assert not q.is_contiguous()
    else:
        q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    if route in ("bshd", "fused"):
        out = ops.attention_bshd(q, k, v, scale, **kw)
    else:
        split = int(route[5:])
        a, b = ops.attention_bshd_split(q, k, v, split, scale, **kw)
        assert a.shape[1] == split and a.is_contiguous() and b.is_contiguous()
        out = torch.cat([a, b], dim=1)
    return out.permute(0, 2, 1, 3)
