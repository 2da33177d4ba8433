"""Attention with a log-sum-exp output, and the merge of partial results:
cases, fp64 references, a plain-torch emulation that takes a ``fault=``, the
bounds and the numbers they were chosen from.

Shared by test_attn_lse_reference.py (CPU: the emulation and ops.* on the
reference path pass every check, every injected fault is rejected by a check
the test names) and test_gpu_attn_lse.py (GPU: the native kernels through the
same checks). The attention cases, the fp64 reference of the output and the
emulation of the output's arithmetic are attention_cases.py's. Everything
here is CPU-only and deterministic.

Every check raises AssertionError with its own name first in the message:
  lse_bound          lse against the fp64 logsumexp, per element
  lse_dead_rows      rows that see no key: lse exactly -inf
  merge_constant     merged constant_columns chunks, bit for bit
  merge_gather       merged one_hot_gather chunks, bit for bit
  merge_skips_dead   a partial with lse = -inf and out = NaN changes nothing
  merge_bound        merged random chunks against fp64, per element
"""
import functools
import math

import torch

import attention_cases as A
import kernel_cases as C
from elementwise_cases import same_bits, spacing16
from comfyui_parallelanything_amd import ops

BF16, F16 = A.BF16, A.F16
LN2 = 0.6931471805599453
NEG_INF = float("-inf")

# Key cuts of Sk = 321: three uneven chunks (one of a single key, none on a
# tile boundary), and eight chunks of 41 (the last 34): one per GPU of a node
CUTS3 = (130, 1, 190)
CUTS8 = (41,) * 7 + (34,)
CUTS = {"3": CUTS3, "8": CUTS8}
assert sum(CUTS3) == sum(CUTS8) == A.SK


# --------------------------------------------------------------------------
# References
# --------------------------------------------------------------------------

def lse64(case, scale=None):
    """fp64 log of the sum over visible keys of exp(scale * q.k), [B,H,Sq];
    -inf on a row that sees no key."""
    q, k = case["q"].double(), case["k"].double()
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    s = (torch.matmul(q, k.transpose(-1, -2)) * scale).masked_fill(
        ~C.visibility(case)[:, None], NEG_INF)
    return torch.logsumexp(s, dim=-1)


def split_keys(case, cuts):
    """The case cut along the keys: one sub-case per chunk, same q."""
    assert case["block"] is None and sum(cuts) == case["k"].shape[2]
    subs, lo = [], 0
    for n in cuts:
        hi = lo + n
        subs.append(dict(
            q=case["q"], k=case["k"][:, :, lo:hi], v=case["v"][:, :, lo:hi],
            keys=None if case["keys"] is None else case["keys"][:, lo:hi],
            block=None))
        lo = hi
    return subs


def dead_batch_case(D, dtype, B=2, H=4):
    """Random data; batch element 1 has no live key, element 0 a Bernoulli
    mask. K/V at dead keys are NaN (don't-care by contract)."""
    case = dict(A.rounding_case("flat_offset", B, H, D, dtype, seed=3))
    keys = torch.rand(B, A.SK, generator=A._gen(77)) < 0.5
    keys[1] = False
    dead = ~keys[:, None, :, None].expand_as(case["k"])
    case["k"] = case["k"].masked_fill(dead, float("nan"))
    case["v"] = case["v"].masked_fill(dead, float("nan"))
    case["keys"] = keys
    return case


# --------------------------------------------------------------------------
# Emulation of the LSE epilogue of attn_fwd_v4_kernel (ops/hip/attention.h):
# the kernel's tile walk and fp32 running (m, l) as attention_cases.emulate
# keeps them (m in the log2 domain, the exp2 argument one fused multiply-
# add), then lse = ln2 * (m + log2 l), -inf where l == 0, stored at
# [b, h, row] or [b, row, h]. Faults:
#   "log2_domain"   lse left in the log2 domain (no ln2)
#   "no_log_l"      log l dropped: ln2 * m
#   "first_tile"    m and l of the first processed tile only
#   "sentinel"      the -1e30 sentinel stored where -inf belongs
#   "bhswap"        batch and head swapped in the lse address
#   "bhs_on_bshd"   the [B, H, S] layout written on a BSHD call
# --------------------------------------------------------------------------

LSE_FAULTS = ("log2_domain", "no_log_l", "first_tile", "sentinel", "bhswap",
              "bhs_on_bshd")


def emulate_lse(case, scale=None, fault=None, bshd=False):
    """fp32 lse as the kernel stores it: [B,H,Sq], or [B,Sq,H] with bshd."""
    q, k = case["q"], case["k"]
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    scale2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(
        A.LOG2E, dtype=torch.float32)
    nq, nk = ops.reference.block_mask_shape(Sq, Sk)
    kf = torch.zeros(B, H, nk * A.KV, D)
    kf[:, :, :Sk] = torch.nan_to_num(k.float())     # dead rows stage as zeros
    qf = q.float()
    tiles = {}
    for b, qb, t, bits in C.processed_tiles(case):
        tiles.setdefault((b, qb), []).append((t, bits))
    m_all = torch.full((B, H, Sq), -1e30)
    l_all = torch.zeros(B, H, Sq)
    for b in range(B):
        for qb in range(nq):
            r0, r1 = qb * A.QB, min(qb * A.QB + A.QB, Sq)
            m_run = torch.full((H, r1 - r0), -1e30)
            l_run = torch.zeros(H, r1 - r0)
            for j, (t, bits) in enumerate(tiles.get((b, qb), [])):
                if fault == "first_tile" and j > 0:
                    break
                kt = kf[b, :, t * A.KV:(t + 1) * A.KV] * bits[None, :, None]
                st = torch.matmul(qf[b, :, r0:r1], kt.transpose(-1, -2))
                if not bool(bits.all()):
                    st = torch.where(bits[None, None, :], st,
                                     torch.tensor(-3e30))
                mnew = torch.maximum(m_run, st.amax(-1) * scale2)
                alpha = torch.exp2(m_run - mnew)
                m_run = mnew
                arg = (st.double() * scale2.double()
                       - mnew[..., None].double()).float()      # one fma
                l_run = l_run * alpha + torch.exp2(arg).sum(-1)
            m_all[b, :, r0:r1] = m_run
            l_all[b, :, r0:r1] = l_run
    live = l_all > 0
    logl = torch.log2(torch.where(live, l_all, torch.ones(())))
    ln2 = torch.tensor(LN2, dtype=torch.float32)
    if fault == "log2_domain":
        lse = m_all + logl
    elif fault == "no_log_l":
        lse = ln2 * m_all
    else:
        lse = ln2 * (m_all + logl)
    dead = torch.tensor(-1e30 if fault == "sentinel" else NEG_INF)
    lse = torch.where(live, lse, dead)
    if fault == "bhswap":
        bb, hh = torch.arange(B)[:, None], torch.arange(H)[None, :]
        lse = lse[hh % B, bb % H]
    if not bshd:
        return lse
    if fault == "bhs_on_bshd":
        return lse.contiguous().view(B, Sq, H)
    return lse.permute(0, 2, 1).contiguous()


# --------------------------------------------------------------------------
# Emulation of attn_merge_kernel (ops/hip/attn_merge.h) in fp32. Faults:
#   "nomax"        weights exp(lse_c) without the maximum subtracted
#   "nonorm"       the weighted sum not divided by the sum of the weights
#   "mul_dead"     a partial with lse = -inf multiplied by its weight 0
#                  instead of skipped
#   "pairwise16"   partials folded pairwise, each fold rounded to 16 bit
#   "skip_last"    the last partial left out
# --------------------------------------------------------------------------

MERGE_FAULTS = ("nomax", "nonorm", "mul_dead", "pairwise16", "skip_last")


def _merge_fp32(outs, lses, fault=None):
    """(fp32 out ahead of the rounding, fp32 lse) of one merge."""
    L = torch.stack(list(lses))
    m = L.amax(0)
    dead = m == NEG_INF
    base = torch.zeros_like(m) if fault == "nomax" else torch.where(
        dead, torch.zeros_like(m), m)
    w = torch.exp(L - base)
    live = L != NEG_INF
    acc = torch.full(outs[0].shape, -0.0)
    wsum = torch.zeros_like(m)
    for c, o in enumerate(outs):
        if fault == "mul_dead":
            acc = acc + w[c][..., None] * o.float()
            wsum = wsum + w[c]
        else:
            acc = torch.where(live[c][..., None],
                              acc + w[c][..., None] * o.float(), acc)
            wsum = torch.where(live[c], wsum + w[c], wsum)
    out = acc if fault == "nonorm" else acc / wsum[..., None]
    out = torch.where(dead[..., None], torch.zeros(()), out)
    lse = torch.where(dead, m, base + torch.log(wsum))
    return out, lse


def emulate_merge(outs, lses, fault=None, return_lse=False):
    outs, lses = list(outs), list(lses)
    dtype = outs[0].dtype
    if fault == "skip_last" and len(outs) > 1:
        outs, lses = outs[:-1], lses[:-1]
    if fault == "pairwise16":
        out, lse = outs[0], lses[0]
        for o, l in zip(outs[1:], lses[1:]):
            out, lse = _merge_fp32([out, o], [lse, l])
            out = out.to(dtype)
    else:
        out, lse = _merge_fp32(outs, lses, fault)
        out = out.to(dtype)
    return (out, lse) if return_lse else out


# --------------------------------------------------------------------------
# The lse bound: |lse - lse64| <= LSE_A + LSE_B * |lse64| per element.
#
# Units from the number formats: the kernel adds log2(l), l in [1, Sk], to m
# and multiplies by ln2; log2(l) < 8.4 has an fp32 spacing of up to 2^-21,
# which nothing downstream can resolve (the absolute unit), and every fp32
# operation on values of lse's size is off by up to 2^-24 of it (the relative
# unit). The multiplier is measured, by SLACK's rule: the worst distance of
# the fp32 emulation from fp64, in those units, over flat_offset and peaked
# at both scales, both grids, D = 64 and 128, bf16 and fp16
# (test_lse_bound_is_twice_the_measured_worst recomputes it), doubled:
#     measured worst   7.97 of (2^-21 + 2^-24 |lse|) (fp16, peaked, scale
#                      0.3, D = 128, the 2-D grid: scores of size 100 summed
#                      in fp32, as for SLACK; default scale stays below 1.04,
#                      bf16 below 2.7)
#     chosen           LSE_A = 2 * 7.97 * 2^-21 = 7.6e-6,
#                      LSE_B = 2 * 7.97 * 2^-24 = 9.5e-7
# Twice the worst covers v_exp_f32, v_log_f32 and the MFMA's summation order,
# which the emulation cannot know.
# --------------------------------------------------------------------------
LSE_UNIT_A = 2.0 ** -21
LSE_UNIT_B = 2.0 ** -24
LSE_MEASURED = 7.97
LSE_A = 2 * LSE_MEASURED * LSE_UNIT_A
LSE_B = 2 * LSE_MEASURED * LSE_UNIT_B


def lse_distance(lse, ref):
    """Worst |lse - ref| in units of (2^-21 + 2^-24 |ref|), finite ref only."""
    fin = torch.isfinite(ref)
    if not fin.any():
        return 0.0
    err = (lse.cpu().double() - ref)[fin].abs()
    return (err / (LSE_UNIT_A + LSE_UNIT_B * ref[fin].abs())).max().item()


def check_lse(lse, ref, what=""):
    """lse [B,H,Sq] fp32 against lse64's ref: exactly -inf where ref is,
    within the bound elsewhere. Returns the worst |err| / bound."""
    lse = lse.cpu()
    assert lse.dtype == torch.float32 and lse.shape == ref.shape, (
        f"lse_bound {what}: {lse.dtype} {tuple(lse.shape)} for fp32 "
        f"{tuple(ref.shape)}")
    dead = ref == NEG_INF
    assert (lse[dead] == NEG_INF).all(), (
        f"lse_dead_rows {what}: a row that sees no key has lse "
        f"{lse[dead][lse[dead] != NEG_INF][0].item()}, not -inf")
    fin = ~dead
    err = (lse.double() - ref)[fin].abs()
    bound = LSE_A + LSE_B * ref[fin].abs()
    # NaN and +-inf fail the comparison
    worst = torch.nan_to_num(err / bound, nan=float("inf")).max().item() \
        if fin.any() else 0.0
    print(f"lse_bound {what}: worst |err|/bound {worst:.4f}")
    assert worst <= 1.0, (
        f"lse_bound {what}: an element is {worst:.4g} of its bound "
        f"{LSE_A:.3g} + {LSE_B:.3g} |lse| from the fp64 logsumexp")
    return worst


def check_dead_out(out, ref, what=""):
    """out [B,H,Sq,D] is +0 bit for bit on every row whose ref lse is -inf."""
    rows = out.cpu()[ref == NEG_INF]
    same_bits(rows, torch.zeros_like(rows), f"lse_dead_rows {what}: out")


# --------------------------------------------------------------------------
# Merge checks
# --------------------------------------------------------------------------

def check_merge_constant(out, case, what=""):
    try:
        A.check_constant(out, case, what)
    except AssertionError as err:
        raise AssertionError(f"merge_constant {what}: {err}") from None


def check_merge_gather(out, case, what=""):
    try:
        assert torch.isfinite(out.float()).all() or not torch.isfinite(
            case["want"].float()).all(), "non-finite output"
        return A.check_gather(out, case, what)
    except AssertionError as err:
        raise AssertionError(f"merge_gather {what}: {err}") from None


def check_merge_skips_dead(merge, outs, lses, what=""):
    """``merge(outs, lses, return_lse=True)`` with one more partial, lse =
    -inf and out = NaN, at the front, in the middle and at the end: the same
    bits as without it."""
    want_o, want_l = merge(outs, lses, return_lse=True)
    nan_o = torch.full_like(outs[0], float("nan"))
    inf_l = torch.full_like(lses[0], NEG_INF)
    for at in (0, len(outs) // 2, len(outs)):
        o, l = merge(outs[:at] + [nan_o] + outs[at:],
                     lses[:at] + [inf_l] + lses[at:], return_lse=True)
        ok = (torch.equal(A._bits(o.cpu()), A._bits(want_o.cpu()))
              and torch.equal(l.cpu(), want_l.cpu()))
        assert ok, (f"merge_skips_dead {what}: a dead partial at {at} of "
                    f"{len(outs)} changed the result "
                    f"({int(torch.isnan(o.float()).sum())} NaN)")


def merge_reference64(case, cuts, scale=None):
    """What the merge bound needs, in fp64: the unsplit reference64, plus
    half_sp = 0.5 sum_c w_c spacing_E(ref_c) and sav = sum_c w_c sav_l_c,
    w_c the chunk weights exp(lse_c - lse), ref_c the chunk results."""
    r = dict(A.reference64(case, scale))
    dtype = case["q"].dtype
    total = lse64(case, scale)
    half_sp = torch.zeros_like(r["ref"])
    sav = torch.zeros_like(r["ref"])
    for sub in split_keys(case, cuts):
        rc = A.reference64(sub, scale)
        w = torch.exp(lse64(sub, scale) - total)[..., None]
        half_sp += 0.5 * w * spacing16(rc["ref"], dtype)
        sav += w * rc["sav_l"]
    r["half_sp"], r["sav"], r["lse"] = half_sp, sav, total
    return r


def merge_distance(out, r, dtype, old=False):
    """Worst |out - ref| over the merge bound
        0.5 spacing_E(ref) + (1 + SLACK) U sum_j P_j |v_j|
            + 0.5 sum_c w_c spacing_E(ref_c)   [+ the fp16 underflow term]:
    attention_cases' bound plus the one rounding each partial has already
    had. old=True leaves that term out (the unsplit kernel's bound)."""
    err = (out.cpu().double() - r["ref"]).abs()
    bound = 0.5 * spacing16(r["ref"], dtype) + (1 + A.SLACK) * A.U[dtype] \
        * r["pav"]
    if not old:
        bound = bound + r["half_sp"]
    if dtype == F16:
        bound = bound + 2.0 ** -25 * r["sav"]
    return torch.nan_to_num(err / bound, nan=float("inf")).max().item()


def check_merge_bound(out, r, dtype, what=""):
    assert out.dtype == dtype, f"merge_bound {what}: {out.dtype}"
    worst = merge_distance(out, r, dtype)
    print(f"merge_bound {what}: worst |err|/bound {worst:.4f}")
    assert worst <= 1.0, (
        f"merge_bound {what}: an element is {worst:.4f} of its bound from "
        f"fp64")
    return worst


# Measured on the CPU emulation at D = 64, B, H = 2, 4, both scales, both
# regimes, bf16 and fp16 (worst |err| / bound;
# test_merge_bound_holds_the_emulation_not_pairwise recomputes them):
#     emulation, this bound    0.53-0.84 (3 chunks), 0.53-0.72 (8 chunks)
#     emulation, old bound     0.73-1.33: above 1.0 three times (peaked at
#                              scale 0.3: bf16 3 chunks 1.33, fp16 3 chunks
#                              1.06, fp16 8 chunks 1.004) - the extra term is
#                              needed
#     pairwise16, this bound   1.43-1.75 at 8 chunks (seven roundings on the
#                              way); 0.68-0.84 at 3 chunks, where two
#                              roundings of partial sums stay inside what
#                              three rounded partials are allowed


@functools.lru_cache(maxsize=None)
def merge_case(regime, grid, D, dtype, scale, cuts):
    """(case, merge_reference64), built once, never modified."""
    case = A.rounding_case(regime, *grid, D, dtype)
    return case, merge_reference64(case, CUTS[cuts], scale)


# --------------------------------------------------------------------------
# A case through ops.attention*_lse on `device` ("cpu": the reference path).
# --------------------------------------------------------------------------

LSE_ROUTES = ("bhsd", "bshd", "fused")


def run_ops_lse(case, route="bhsd", device="cpu", scale=None, plain=False):
    """(out [B,H,Sq,D], lse [B,H,Sq]) whatever the route's layout; the routes
    are attention_cases.run_ops's. plain=True calls ops.attention* instead
    and returns its out alone."""
    def dev(t):
        return None if t is None else t.to(device)

    q, k, v = (dev(case[n]) for n in "qkv")
    kw = dict(key_mask=dev(case["keys"]))
    if route == "bhsd":
        if plain:
            return ops.attention(q, k, v, scale, **kw)
        out, lse = ops.attention_lse(q, k, v, scale, **kw)
        assert lse.shape == out.shape[:-1] and lse.is_contiguous()
        return out, lse
    if route == "fused":
        buf = torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], dim=2)
        q, k, v = buf.unbind(2)
        assert not q.is_contiguous()
    else:
        q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    if plain:
        return ops.attention_bshd(q, k, v, scale, **kw).permute(0, 2, 1, 3)
    out, lse = ops.attention_bshd_lse(q, k, v, scale, **kw)
    assert lse.shape == out.shape[:-1] and lse.is_contiguous()
    return out.permute(0, 2, 1, 3), lse.permute(0, 2, 1)


def chunk_partials(case, cuts, device="cpu", scale=None, bshd=False):
    """ops.attention[_bshd]_lse over each key chunk: (outs, lses), lists of
    contiguous tensors in the call's own layout."""
    outs, lses = [], []
    for sub in split_keys(case, cuts):
        q, k, v = (sub[n].to(device) for n in "qkv")
        km = None if sub["keys"] is None else sub["keys"].to(device)
        if bshd:
            q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
            o, l = ops.attention_bshd_lse(q, k, v, scale, key_mask=km)
        else:
            o, l = ops.attention_lse(q, k, v, scale, key_mask=km)
        outs.append(o)
        lses.append(l)
    return outs, lses


def emulated_partials(case, cuts, scale=None):
    """The emulation's partials over each key chunk, [B,H,Sq,D] / [B,H,Sq]."""
    subs = split_keys(case, cuts)
    return ([A.emulate(s, scale) for s in subs],
            [emulate_lse(s, scale) for s in subs])
