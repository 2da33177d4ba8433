"""Inputs, byte-exact references and checks for the fp8 (e4m3fn) emit kernels
(ops/hip/fp8.h): quant_fp8, gelu_fp8, layer_norm_mod_fp8 and the delayed-
scaling finalize.

Shared by test_fp8_cases_reference.py (CPU: a plain-torch emulation of the
kernels stands in for them, the faithful one passes every check and every
injected fault is rejected by a named one) and test_gpu_fp8_exact.py (GPU:
the same checks on the real kernels). Everything here is CPU-only and
deterministic. A check is a function of a backend, an object with

    quant(x, st) / gelu(x, st) / ln(x, sc, sh, st)   -> uint8 bytes (CPU)
    large(op, pattern, nvec, st)                     -> uint8 [nvec, 8]

that runs one call of the op on CPU tensors and leaves the state it produced
in `st` (a DelayedScale used as a plain holder of scale / amax_buf /
scale_used).

Why not rel-l2 < 0.05 on randn: on such data a correct cast gives 0.0265,
and so does one that flushes every subnormal code; one element in five a
code too high gives 0.0494. Ties, -0, the subnormal codes and the saturation
edge need inputs that sit on them, and a byte comparison.
"""
import math

import torch

import kernel_cases as C

E4M3 = torch.float8_e4m3fn
BF16 = torch.bfloat16
F32 = torch.float32
U8 = torch.uint8


def f32(v):
    return torch.tensor(v, dtype=F32)


# --------------------------------------------------------------------------
# The e4m3fn grid: all 256 bytes decoded through torch. Bytes 0x00 .. 0x7e
# are 0, the seven subnormals k * 2^-9, and the normals up to 448, ascending;
# 0x7f and 0xff are NaN; bit 7 is the sign.
# --------------------------------------------------------------------------

ALL_BYTES = torch.arange(256, dtype=torch.int64).to(U8)
GRID = ALL_BYTES.view(E4M3).float()
FINITE_BYTES = ALL_BYTES[(ALL_BYTES & 0x7F) != 0x7F]          # 254 codes
POS = GRID[:127].double()                                     # 0 .. 448
# where the rounded code changes: the midpoints of adjacent codes, and 464,
# the midpoint of 448 and the 480 that e4m3fn gives to NaN
BOUNDARIES = torch.cat([(POS[:-1] + POS[1:]) / 2,
                        torch.tensor([464.0], dtype=torch.float64)])
NAN_BYTE = 0x7F
MAX_BYTE = 0x7E                                               # +448


def is_nan_byte(b):
    return (b & 0x7F) == 0x7F


def spacing(v):
    """Distance between adjacent codes around |v|: 2^(floor(log2|v|) - 3),
    and 2^-9 below 2^-6 (the subnormal codes)."""
    a = v.double().abs().clamp(min=2.0 ** -6, max=1e30)
    _, e = torch.frexp(a)                     # a = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), e - 1 - 3)


def encode(v, rounding="rne", clamp=448.0, flush_subnormals=False,
           keep_neg_zero=True):
    """e4m3fn byte of each v (any float type, taken as fp64) by walking the
    grid: an encoder independent of torch's cast, exact for fp64 inputs, and
    with the knobs the injected faults need. rounding: "rne", "away" (ties
    away from zero), "truncate" (toward zero), "ceil" (away from zero).
    clamp=None is the bare OCP cast: beyond 464 it gives NaN."""
    v = v.double()
    nan = v.isnan()
    neg = torch.signbit(v)
    a = torch.where(nan, torch.zeros_like(v), v.abs())
    over = a > 464.0
    if clamp is not None:
        a = a.clamp(max=clamp)
    a = a.clamp(max=448.0)
    lo = (torch.searchsorted(POS, a, right=True) - 1).clamp(0, 126)
    hi = (lo + 1).clamp(max=126)
    dl, dh = a - POS[lo], POS[hi] - a
    if rounding == "rne":
        up = (dh < dl) | ((dh == dl) & (lo % 2 == 1))
    elif rounding == "away":
        up = dh <= dl
    elif rounding == "ceil":
        up = dl > 0
    else:
        up = torch.zeros_like(nan)
    code = torch.where(up & (hi > lo), hi, lo)
    if flush_subnormals:
        code = torch.where(code < 8, torch.zeros_like(code), code)
    byte = code + 128 * neg.long()
    if not keep_neg_zero:
        byte = torch.where(code == 0, torch.zeros_like(byte), byte)
    if clamp is None:
        byte = torch.where(over, torch.full_like(byte, NAN_BYTE), byte)
    byte = torch.where(nan, torch.full_like(byte, NAN_BYTE), byte)
    return byte.to(U8)


def emit_bytes(y, scale):
    """The byte-exact reference of out = fp8(y / scale[0]): inv = fp32(1) /
    scale and v = y * inv in fp32, clamp to +-448, torch's CPU cast (round
    to nearest even, subnormals included). NaN gives a NaN byte, +-inf
    +-448."""
    inv = torch.ones((), dtype=F32) / scale.to(F32).reshape(())
    v = y.to(F32) * inv
    return v.clamp(-448.0, 448.0).to(E4M3).view(U8)


def scaled64(y64, scale):
    """The exact value the cast sees, up to the kernel's own error in y: y
    in fp64 times the fp32 reciprocal the kernel multiplies by."""
    inv = (torch.ones((), dtype=F32) / scale.to(F32).reshape(())).double()
    return y64.double() * inv


# A fused kernel computes y in fp32 with approximations (v_exp, v_rcp, fp32
# row statistics), so its y differs from the fp64 one and, next to a
# rounding boundary, so may its byte. The margin was set for kernels good to
# 1e-4 relative: a spacing is at least 1/16 of the value, so such an error is
# below 2e-3 spacings and 1/64 leaves a factor of eight. That holds where
# the value is a product; where it is a difference of larger terms the error
# is measured in spacings of the small result (see LN_CASES and gelu_f32).
MARGIN = 1.0 / 64
EXCLUDED_CAP = 0.05


def offtie_mask(v64, margin=MARGIN):
    """True where v64 lies further than `margin` spacings from every
    rounding boundary (the 448|464 edge counts as one). NaN is False. The
    byte holds a sign, so for a v64 that is not itself zero, zero is a
    boundary too: 0x00 on one side, 0x80 on the other."""
    a = v64.double().abs().clamp(max=1e30)
    i = torch.searchsorted(BOUNDARIES, a).clamp(1, len(BOUNDARIES) - 1)
    d = torch.minimum((a - BOUNDARIES[i - 1]).abs(),
                      (a - BOUNDARIES[i]).abs())
    d = torch.minimum(d, (a - BOUNDARIES[0]).abs())
    d = torch.where(a > 0, torch.minimum(d, a), d)
    return (d > margin * spacing(a)) & ~v64.isnan()


def excluded_share(v64, margin=MARGIN):
    """Share of the in-range elements (2^-10 <= |v| <= 464) that
    offtie_mask leaves out."""
    a = v64.double().abs()
    inr = (a >= 2.0 ** -10) & (a <= 464.0)
    return ((~offtie_mask(v64, margin)) & inr).sum().item() / max(
        inr.sum().item(), 1)


def same_bytes(got, want, what=""):
    """Byte equality; where the reference is NaN either NaN byte will do."""
    got, want = got.flatten(), want.flatten()
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    nan = is_nan_byte(want)
    bad = torch.where(nan, ~is_nan_byte(got), got != want)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} bytes differ, first "
            f"at {i}: got 0x{int(got[i]):02x}, want 0x{int(want[i]):02x}")


def check_offtie(got, v64, what="", margin=MARGIN):
    """The off-tie criterion: where v64 is clear of every boundary the byte
    is that of v64 rounded to nearest even; elsewhere it is one of the two
    neighbouring codes; NaN gives a NaN byte."""
    got, v64 = got.flatten(), v64.flatten().double()
    assert got.shape == v64.shape, f"{what}: {got.shape} vs {v64.shape}"
    nan = v64.isnan()
    clear = offtie_mask(v64, margin)
    want = encode(v64)
    bad = clear & (got != want)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {int(clear.sum())} off-tie bytes "
            f"differ, first at {i}: v = {v64[i].item()!r}, got "
            f"0x{int(got[i]):02x}, want 0x{int(want[i]):02x}")
    near = ~clear & ~nan
    ok = (got == encode(v64, "truncate")) | (got == encode(v64, "ceil"))
    ok |= ((got & 0x7F) == 0) & (v64.abs() <= margin * 2.0 ** -9)
    assert ok[near].all(), f"{what}: a byte next to a tie is no neighbour"
    assert is_nan_byte(got[nan]).all(), f"{what}: NaN in, no NaN byte out"


# --------------------------------------------------------------------------
# DelayedScale: the state machine of fp8_scale_finalize_kernel in fp32 torch
# ops, each one rounding as the kernel's three do.
#   used  = scale
#   amax  = fp32(max(amax, cur) * 0.999f)
#   scale = max(amax / 448, 1e-12)
# A one-slot amax_buf only maxes. A running amax that is not finite never
# reaches the scale: scale stays, amax = scale * 448, used is snapshotted as
# always. Also the plain holder of the three tensors a backend fills in.
# --------------------------------------------------------------------------

STATE_FAULTS = ("amax_overwritten", "no_decay", "scale_undecayed",
                "late_snapshot", "no_floor", "inf_accepted")


class DelayedScale:
    def __init__(self, scale, amax=0.0, slots=2, aliased=False):
        self.scale = torch.tensor([scale], dtype=F32)
        self.amax = torch.zeros(slots, dtype=F32)
        self.amax[0] = amax
        self.aliased = aliased
        self.used = self.scale if aliased else torch.zeros(1, dtype=F32)

    def clone(self):
        c = DelayedScale(0.0, 0.0, self.amax.numel(), self.aliased)
        c.scale.copy_(self.scale)
        c.amax.copy_(self.amax)
        if not self.aliased:
            c.used.copy_(self.used)
        return c

    def update(self, cur, fault=None):
        """One call whose values have the maximum magnitude `cur` (fp32)."""
        cur = cur.to(F32).reshape(())
        m = cur if fault == "amax_overwritten" else torch.maximum(
            self.amax[0], cur)
        if self.amax.numel() < 2:
            self.amax[0] = m
            return self
        if not self.aliased:
            self.used.copy_(self.scale)
        if not torch.isfinite(m) and fault != "inf_accepted":
            self.amax[0] = self.scale[0] * f32(448.0)
            return self
        nxt = m if fault == "no_decay" else m * f32(0.999)
        self.amax[0] = nxt
        new = (m if fault == "scale_undecayed" else nxt) / f32(448.0)
        if fault != "no_floor":
            new = torch.maximum(new, f32(1e-12))
        self.scale[0] = new
        if fault == "late_snapshot" and not self.aliased:
            self.used.copy_(self.scale)
        return self

    def __repr__(self):
        return (f"scale={self.scale.tolist()} amax={self.amax.tolist()} "
                f"used={self.used.tolist()}")


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_state(got, want, what=""):
    """scale, amax_buf and scale_used bit for bit."""
    for name in ("scale", "amax", "used"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), \
            f"{what}: {name} got [{got}] want [{want}]"


def amax_of(y):
    """fp32 max |y| as the kernels take it: from 0, NaN skipped."""
    a = y.to(F32).abs().flatten()
    a = torch.where(a.isnan(), torch.zeros_like(a), a)
    return torch.cat([a, torch.zeros(1)]).max()


AMAX_REL = 1e-5


def check_fused_state(st, entry, y64, what=""):
    """State after a fused op whose amax comes from the kernel's own fp32
    values: amax_buf[0] within AMAX_REL of what the fp64 maximum gives
    (bit-exact where that leaves no room, as under a larger prior amax or
    the non-finite rule), scale == max(amax_after / 448, 1e-12) bitwise,
    scale_used == the entry scale bitwise, slot 1 zero."""
    a = y64.double().abs().flatten()
    cur = torch.cat([torch.where(a.isnan(), torch.zeros_like(a), a),
                     torch.zeros(1, dtype=torch.float64)]).max()
    lo = entry.clone().update((cur * (1 - AMAX_REL)).to(F32))
    hi = entry.clone().update((cur * (1 + AMAX_REL)).to(F32))
    if torch.equal(_bits(lo.amax), _bits(hi.amax)):
        return same_state(st, lo, what)
    assert lo.amax[0] <= st.amax[0] <= hi.amax[0], \
        f"{what}: amax {st.amax[0].item()!r} outside " \
        f"[{lo.amax[0].item()!r}, {hi.amax[0].item()!r}]"
    assert st.amax[1] == 0, what
    want = torch.maximum(st.amax[0] / f32(448.0), f32(1e-12)).reshape(1)
    assert torch.equal(_bits(st.scale), _bits(want)), \
        f"{what}: scale {st.scale.item()!r}, amax/448 = {want.item()!r}"
    assert torch.equal(_bits(st.used), _bits(entry.scale)), \
        f"{what}: used {st.used.item()!r}, entry {entry.scale.item()!r}"


# --------------------------------------------------------------------------
# Inputs (bf16, CPU, a multiple of 8 long). Values are given in units of the
# code grid and multiplied by UNIT = 2^-7, which is exact, so at scale 2^-7
# the kernel's y * inv is the grid value itself.
# --------------------------------------------------------------------------

UNIT = 2.0 ** -7
SCALES = {"2^-7": UNIT, "0.012": 0.012, "0.37": 0.37, "floor": 1e-12}


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bf16_next(x, step):
    """The bf16 value `step` bit patterns further from zero."""
    return (x.view(torch.int16) + step).view(BF16)


def _pad8(x, fill):
    pad = (-x.numel()) % 8
    return torch.cat([x, torch.full((pad,), fill, dtype=x.dtype)])


def every_code():
    """Each of the 254 finite codes times 2^-7 (exact in bf16, -0 included),
    then two 1.0 codes: at scale 2^-7 the output bytes are FINITE_BYTES."""
    v = GRID[FINITE_BYTES.long()] * UNIT
    x = _pad8(v, UNIT).to(BF16)
    assert torch.equal(x.float()[:254], v)
    return x


def ties():
    """Every tie between adjacent codes (2^-10, the tie of 0 and the first
    subnormal, and the six other subnormal ties included) and the bf16
    values just below and above it, both signs."""
    t = (BOUNDARIES[:-1] * UNIT).to(BF16)
    assert torch.equal(t.double(), BOUNDARIES[:-1] * UNIT)
    x = torch.cat([_bf16_next(t, -1), t, _bf16_next(t, 1)])
    return _pad8(torch.cat([x, -x]), 0.0)


def saturation_edge():
    v = torch.tensor([448.0, 449.0, 464.0, 465.0, 1e4,
                      torch.finfo(BF16).max * 2.0 ** 7, math.inf])
    x = (v * UNIT).to(BF16)
    return _pad8(torch.cat([x, -x]), UNIT)


def all_bf16():
    """All 65536 bit patterns: +-0, subnormals, +-inf and every NaN."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)


def all_finite_bf16():
    x = all_bf16()
    return x[torch.isfinite(x.float())]                  # 65280 = 8 * 8160


QUANT_INPUTS = {"every_code": every_code, "ties": ties,
                "saturation_edge": saturation_edge, "all_bf16": all_bf16}

# ---- the large launch -----------------------------------------------------
# fp8_emit_loop runs a grid of at most 4096 blocks x 256 threads, each
# thread taking vectors first + (4 * trip + slot) * GRID_VECS. LARGE_NVEC is
# the smallest size with a second trip: thread t holds slots 0..3 of trip 0
# and slot 0 (five threads also slot 1) of trip 1. The data has a period of
# 8191 vectors, a prime, coprime to GRID_VECS = 2^20: the vectors of one
# thread are 2^20 apart, so no two of them hold the same pattern row.

GRID_VECS = 4096 * 256
LARGE_NVEC = GRID_VECS * 5 + 5
PERIOD = 8191


def large_pattern():
    """[PERIOD, 8] bf16, rows pairwise different, about a tenth of the
    values beyond +-448 at scale 2^-7."""
    x = torch.randn(PERIOD, 8, generator=_gen(8191)) * (270.0 * UNIT)
    return x.to(BF16)


def large_mismatches(got, want_pat, clear_pat=None):
    """Vectors of got [nvec, 8] (uint8, any device) that differ from the
    tiled pattern bytes. With clear_pat (the off-tie mask of the pattern)
    only clear elements are held to want_pat, and every element to the
    first period of got itself, which check_offtie then judges."""
    idx = torch.arange(got.shape[0], device=got.device) % PERIOD
    bad = got != want_pat.to(got.device)[idx]
    if clear_pat is not None:
        bad &= clear_pat.to(got.device)[idx]
        bad |= got != got[:PERIOD][idx]
    return int(bad.any(1).sum())


# ---- state inputs ---------------------------------------------------------

BLOCK = 256 * 8                       # elements of one 256-thread block
STATE_N = 3 * BLOCK + 5 * 8           # three full blocks and a partial one
SEQ_AMPS = (1.0, 3.0, 0.5, 0.5, 10.0, 0.0)


def seq_base():
    return torch.randn(STATE_N, generator=_gen(21)).to(BF16)


PEAK = -4.0                           # the maximum is a negative value
PRIOR_PEAKS = {"first": (PEAK, 2.0, 1.0, 3.0),
               "middle": (1.0, PEAK, 2.0, 3.0),
               "last": (1.0, 2.0, 3.0, PEAK)}
PRIOR_LEVELS = {"below": 0.5, "between": 2.5, "above": 5.0}


def prior_input(pos):
    """Four blocks of |x| < 0.9 with one peak each: the largest, -4, in the
    first, a middle or the last (partial) block, the others 1, 2 and 3."""
    x = (0.25 * torch.randn(STATE_N, generator=_gen(22))).clamp(-0.9, 0.9)
    for b, p in enumerate(PRIOR_PEAKS[pos]):
        x[b * BLOCK + (13 if b == 3 else 77 * (b + 1) + 300 * b)] = p
    return x.to(BF16)


# ---- fused-op values ------------------------------------------------------

def gelu_f64(x):
    xd = x.double()
    return 0.5 * xd * (1.0 + torch.tanh(
        math.sqrt(2.0 / math.pi) * (xd + 0.044715 * xd ** 3)))


def gelu_f32(x, cancelling=False):
    """gelu_tanh_f32<true> of ops/hip/elementwise.h, step by step in fp32:
    the negative side takes En * r. cancelling=True is the 1 - r form that
    gelu_tanh keeps and gelu_fp8 had: up to 0.0185 spacings off at scale
    2^-7 (x = -4.97), more than the whole margin."""
    f = x.to(F32)
    c = f32(0.7978845608028654) * (f + f32(0.044715) * f * f * f)
    en = torch.exp2(f32(-2.8853900817779268) * c.abs())
    r = 1.0 / (1.0 + en)
    return f * torch.where(c >= 0, r, 1.0 - r if cancelling else en * r)


GELU_SCALES = ("2^-7", "0.012", "0.37")

LN_SHAPES = ((1, 1, 8), (2, 3, 8 * 257), (2, 5, 3072))
LN_ROWS = ("plain", "offset", "outlier")
LN_EPS = 1e-6
# The modulation the cases need is "subnormal": 1 + scale = k * 2^-8, so the
# outputs fall in the subnormal codes at qscale 1. "plain" (randn scale and
# shift, the largest output at 448) adds the upper codes, where it is sound:
# f * (1 + scale) + shift cancels, and the absolute error of the larger term
# is then measured in spacings of the small result.
# - offset rows: a mean of 40 is an fp32 value, good to 2e-6, and x - mean
#   inherits that whole: 6e-6 absolute after a modulation of 3, which is
#   0.019 of a subnormal spacing at qscale 2^-3 and 0.07 with the largest
#   output at 448. So offset rows run "subnormal" only, where 1 + scale is
#   0.016 at most (2e-5 spacings). With the variance reduced in fp32, as
#   before these tests, the same rows were 0.56 and 1.3 spacings off.
# - plain and outlier rows: fp32 rounding of terms up to 10 is 1e-6
#   absolute, so qscale is at least 2^-3: a subnormal spacing is then 2.4e-4
#   and the error 1/256 of it or less.
# test_fp8_cases_reference.py holds the emulation to a quarter of the margin
# on every case.
LN_CASES = tuple((shape, rows, mod) for shape in LN_SHAPES
                 for rows in LN_ROWS for mod in ("subnormal", "plain")
                 if not (rows == "offset" and mod == "plain"))
MIN_PLAIN_QSCALE = 2.0 ** -3


def ln_modulation(B, D, mod, seed):
    """plain: randn scale and shift. subnormal: 1 + scale = k * 2^-8 with k
    in 1..4 (bf16 is that fine next to -1) and a shift of a few 2^-9."""
    if mod == "plain":
        return C.modulation(B, D, BF16, seed)
    g = _gen(seed)
    k = torch.randint(1, 5, (B, D), generator=g).float()
    sh = torch.randn(B, D, generator=g) * 2.0 ** -8
    return (-1.0 + k * 2.0 ** -8).to(BF16), sh.to(BF16)


def plain_qscale(y64):
    """The largest output at 448, but at least MIN_PLAIN_QSCALE."""
    return max((y64.abs().max() / 448.0).to(F32).item(), MIN_PLAIN_QSCALE)


def ln_case(shape, rows, mod, seed=None):
    """(x [B, S, D], scale [B, D], shift [B, D], qscale)."""
    B, S, D = shape
    seed = D + 7 * LN_ROWS.index(rows) if seed is None else seed
    x = C.norm_rows(rows, B * S, D, BF16, seed).view(B, S, D)
    sc, sh = ln_modulation(B, D, mod, seed + 1)
    if mod == "subnormal":
        return x, sc, sh, 1.0
    return x, sc, sh, plain_qscale(C.layer_norm_mod_f64(x, sc, sh, LN_EPS))


def ln_f32(x, sc, sh, eps=LN_EPS, fused=True, wide=True):
    """layer_norm_mod_fp8_kernel's values: the single-pass row statistics of
    kernel_cases.emulate_row_stats (fused: x * x + s rounded once; wide:
    reduced across the block in fp64, as the kernel does since these tests,
    or in fp32, as it did), then (x - mean) * rstd * (1 + scale) + shift in
    fp32."""
    B, S, D = x.shape
    mean, rstd, _ = C.emulate_row_stats(x.reshape(B * S, D), eps,
                                        fused=fused, wide=wide)
    f = (x.float() - mean.view(B, S, 1)) * rstd.view(B, S, 1)
    return f * (1.0 + sc.float()[:, None]) + sh.float()[:, None]


def ln_prior_case(pos):
    """[2, 3, 8 * 257] randn rows with one outlier row, the first or the
    last: that row's block holds the maximum."""
    B, S, D = 2, 3, 8 * 257
    x = C.plain(B * S, D, BF16, 31)
    x[0 if pos == "first" else B * S - 1, 100] = 40.0
    sc, sh = ln_modulation(B, D, "plain", 32)
    return x.view(B, S, D), sc, sh


# --------------------------------------------------------------------------
# Emulation of the kernels with a fault. The values y are the op's fp32
# results (quant: x itself; gelu: gelu_f32; ln: ln_f32); the emit is y *
# fp32(1 / scale), clamp, cast, with the block amax maxed into the state.
# --------------------------------------------------------------------------

CAST_FAULTS = ("truncate", "ties_away", "subnormals_flushed", "no_clamp",
               "clamp_240", "nan_to_min", "neg_zero_lost")
INDEX_FAULTS = ("last_vector_skipped", "ilp_slot_skipped",
                "ilp_slots_swapped")
AMAX_FAULTS = ("amax_no_abs", "snan_resets_amax")
FAULTS = CAST_FAULTS + AMAX_FAULTS + STATE_FAULTS + INDEX_FAULTS


def _cast(v, fault):
    if fault == "nan_to_min":              # fminf(fmaxf(NaN, -448), 448)
        v = torch.where(v.isnan(), torch.full_like(v, -448.0), v)
    if fault == "truncate":
        return encode(v, "truncate")
    if fault == "ties_away":
        return encode(v, "away")
    if fault == "subnormals_flushed":
        return encode(v, flush_subnormals=True)
    if fault == "no_clamp":
        return encode(v, clamp=None)
    if fault == "clamp_240":               # the fnuz maximum
        return encode(v, clamp=240.0)
    if fault == "neg_zero_lost":
        return encode(v, keep_neg_zero=False)
    return v.clamp(-448.0, 448.0).to(E4M3).view(U8)


def emulate_emit(y, st, fault=None):
    """One launch over the fp32 values y (flat, a multiple of 8) below
    GRID_VECS vectors, where every thread holds at most one vector and the
    ILP faults have nothing to act on. Returns the bytes, updates st."""
    y = y.to(F32).flatten()
    assert y.numel() % 8 == 0 and y.numel() // 8 <= GRID_VECS
    inv = torch.ones((), dtype=F32) / st.scale[0]
    out = _cast(y * inv, fault)
    seen = y
    if fault == "last_vector_skipped":
        out[-8:] = 0
        seen = y[:-8]
    cur = amax_of(seen)
    if fault == "amax_no_abs":
        cur = torch.where(seen.isnan(), torch.zeros_like(seen), seen).max(
            ).clamp(min=0.0)
    if fault == "snan_resets_amax":
        # v_max_f32 in IEEE mode turns a signaling NaN into a quiet one,
        # which the next value replaces: what a thread saw before the last
        # signaling NaN of its vector is lost (quant_fp8 before these tests)
        bits = seen.view(torch.int32).view(-1, 8)
        snan = seen.isnan().view(-1, 8) & ((bits & 0x00400000) == 0)
        later = snan.flip(1).cumsum(1).flip(1) > 0
        cur = amax_of(torch.where(later, torch.zeros(()), seen.view(-1, 8)))
    st.update(cur, fault)
    return out


def large_sources(nvec, fault=None):
    """Which input vector each output vector of a large launch holds (-1:
    never written), by the thread / trip / slot layout of fp8_emit_loop."""
    i = torch.arange(nvec)
    slot = (i // GRID_VECS) % 4
    src = i.clone()
    if fault == "ilp_slot_skipped":
        src[slot == 2] = -1
    if fault == "ilp_slots_swapped":       # slots 1 and 2 of a trip
        j = torch.where(slot == 1, i + GRID_VECS,
                        torch.where(slot == 2, i - GRID_VECS, i))
        src = torch.where(j < nvec, j, i)
    if fault == "last_vector_skipped":
        src[-1] = -1
    return src


class Emulated:
    """The backend of the CPU file: plain torch, with an optional fault."""

    def __init__(self, fault=None):
        self.fault = fault

    def quant(self, x, st):
        return emulate_emit(x.float(), st, self.fault)

    def gelu(self, x, st):
        return emulate_emit(gelu_f32(x), st, self.fault)

    def ln(self, x, sc, sh, st):
        return emulate_emit(ln_f32(x, sc, sh), st, self.fault)

    def large(self, op, pattern, nvec, st):
        y = pattern.float() if op == "quant" else gelu_f32(pattern)
        rows = emulate_emit(y, st.clone(), self.fault).view(PERIOD, 8)
        src = large_sources(nvec, self.fault)
        out = rows[src.clamp(min=0) % PERIOD]
        out[src < 0] = 0
        fault = self.fault if self.fault not in INDEX_FAULTS else None
        st.update(amax_of(y), fault)
        return out


# --------------------------------------------------------------------------
# The checks. Each takes a backend and raises AssertionError.
# --------------------------------------------------------------------------

def _quant_bytes(case, scale_name):
    def check(be):
        what = f"quant {case} scale={scale_name}"
        x = QUANT_INPUTS[case]()
        st = DelayedScale(SCALES[scale_name])
        ref = st.clone()
        got = be.quant(x, st)
        same_bytes(got, emit_bytes(x, ref.scale), what)
        same_state(st, ref.update(amax_of(x)), what)
        if case == "every_code" and scale_name == "2^-7":
            assert torch.equal(got[:254], FINITE_BYTES), what
    return check


def quant_sequence(be):
    """Six calls on one state: x1, x3, x0.5, x0.5, x10 (must saturate) and
    all zeros; bytes and the whole state after every call."""
    base = seq_base().float()
    st = DelayedScale((base.abs().max() / 448.0).item())
    ref = st.clone()
    for n, amp in enumerate(SEQ_AMPS):
        what = f"quant sequence call {n} (x{amp})"
        x = (base * amp).to(BF16)
        got = be.quant(x, st)
        same_bytes(got, emit_bytes(x, ref.scale), what)
        same_state(st, ref.update(amax_of(x)), what)
        if amp == 10.0:
            assert not is_nan_byte(got).any(), what
            assert ((got & 0x7F) == MAX_BYTE).float().mean() > 0.05, what


def _quant_prior(pos, level):
    def check(be):
        what = f"quant prior {pos} {level}"
        x = prior_input(pos)
        st = DelayedScale(-PEAK / 448.0, amax=PRIOR_LEVELS[level])
        ref = st.clone()
        got = be.quant(x, st)
        same_bytes(got, emit_bytes(x, ref.scale), what)
        same_state(st, ref.update(amax_of(x)), what)
    return check


def quant_one_slot(be):
    """A one-slot amax_buf only accumulates: no decay, scale untouched."""
    x = prior_input("middle")
    for prior in (0.5, 5.0):
        st = DelayedScale(0.01, amax=prior, slots=1)
        ref = st.clone()
        got = be.quant(x, st)
        same_bytes(got, emit_bytes(x, ref.scale), "quant one_slot")
        same_state(st, ref.update(amax_of(x)), "quant one_slot")
        assert st.amax[0] == max(prior, -PEAK) and st.scale[0] == f32(0.01)


def quant_aliased(be):
    """scale_used aliased to scale: no snapshot, two calls."""
    x = prior_input("last")
    st = DelayedScale(0.012, aliased=True)
    ref = st.clone()
    for n in range(2):
        got = be.quant(x, st)
        same_bytes(got, emit_bytes(x, ref.scale), f"quant aliased call {n}")
        same_state(st, ref.update(amax_of(x)), f"quant aliased call {n}")


def quant_floor(be):
    """A fresh state fed zeros reaches the 1e-12 floor; the next small
    nonzero call saturates cleanly."""
    st = DelayedScale(0.01)
    ref = st.clone()
    zeros = torch.zeros(STATE_N, dtype=BF16)
    got = be.quant(zeros, st)
    assert not got.any(), "quant floor: zeros"
    same_state(st, ref.update(f32(0.0)), "quant floor: zeros")
    assert st.scale[0] == f32(1e-12) and st.amax[0] == 0
    base = seq_base().float()
    x = ((base + torch.sign(base)) * 1e-6).to(BF16)
    x[::5] = 0.0
    got = be.quant(x, st)
    same_bytes(got, emit_bytes(x, ref.scale), "quant floor: small")
    same_state(st, ref.update(amax_of(x)), "quant floor: small")
    nz = x.float() != 0
    assert ((got & 0x7F) == MAX_BYTE)[nz].all() and not (got & 0x7F)[~nz].any()


def quant_nonfinite(be):
    """An inf element: that call saturates it, the scale stays, the amax
    restarts at scale * 448, and the next finite call is DelayedScale's.
    The same from a prior amax that is already inf or NaN."""
    x = seq_base()
    bad = x.clone()
    bad[5], bad[BLOCK + 9], bad[-1] = math.inf, -math.inf, math.nan
    for prior in (3.0, math.inf, math.nan):
        what = f"quant nonfinite prior={prior}"
        st = DelayedScale(0.02, amax=prior)
        ref = st.clone()
        got = be.quant(bad if prior == 3.0 else x, st)
        same_bytes(got, emit_bytes(bad if prior == 3.0 else x, ref.scale),
                   what)
        same_state(st, ref.update(f32(math.inf)), what)
        assert st.scale[0] == f32(0.02) and st.used[0] == f32(0.02), what
        assert st.amax[0] == f32(0.02) * f32(448.0), what
        if prior == 3.0:
            assert got[5] == MAX_BYTE and got[BLOCK + 9] == 0xFE
            assert is_nan_byte(got[-1])
        got = be.quant(x, st)
        same_bytes(got, emit_bytes(x, ref.scale), what + ", then finite")
        same_state(st, ref.update(amax_of(x)), what + ", then finite")
        assert torch.isfinite(st.scale).all() and torch.isfinite(st.amax).all()


def _large(op):
    def check(be):
        what = f"large {op}"
        pat = large_pattern()
        st = DelayedScale(UNIT)
        ref = st.clone()
        got = be.large(op, pat, LARGE_NVEC, st)
        assert got.shape == (LARGE_NVEC, 8), what
        if op == "quant":
            want = emit_bytes(pat, ref.scale)
            assert large_mismatches(got, want) == 0, what
            same_state(st, ref.update(amax_of(pat)), what)
        else:
            v64 = scaled64(gelu_f64(pat), ref.scale)
            assert large_mismatches(got, encode(v64), offtie_mask(v64)) == 0, \
                what
            check_offtie(got[:PERIOD].cpu(), v64, what)
            check_fused_state(st, ref, gelu_f64(pat), what)
    return check


def _gelu_all(scale_name):
    def check(be):
        what = f"gelu all_finite_bf16 scale={scale_name}"
        x = all_finite_bf16()
        st = DelayedScale(SCALES[scale_name])
        ref = st.clone()
        got = be.gelu(x, st)
        y64 = gelu_f64(x)
        check_offtie(got, scaled64(y64, ref.scale), what)
        check_fused_state(st, ref, y64, what)
    return check


def gelu_nan_inf(be):
    """NaN -> a NaN byte, +inf -> 0x7e, and the non-finite rule on the
    state. (-inf is gelu_tanh's own test's.)"""
    x = torch.tensor([math.nan, math.inf, 1.0, -1.0, 0.0, -0.0, 3.0, -3.0,
                      0.5, -0.5, 2.0, -2.0, 6.0, -6.0, 0.1, -0.1]).to(BF16)
    st = DelayedScale(UNIT, amax=1.0)
    ref = st.clone()
    got = be.gelu(x, st)
    assert is_nan_byte(got[0]) and got[1] == MAX_BYTE, "gelu nan_inf"
    check_offtie(got, scaled64(gelu_f64(x), ref.scale), "gelu nan_inf")
    same_state(st, ref.update(f32(math.inf)), "gelu nan_inf")
    assert st.scale[0] == f32(UNIT)


def _ln(shape, rows, mod):
    def check(be):
        what = f"ln {shape} {rows} {mod}"
        x, sc, sh, qscale = ln_case(shape, rows, mod)
        st = DelayedScale(qscale)
        ref = st.clone()
        got = be.ln(x, sc, sh, st)
        y64 = C.layer_norm_mod_f64(x, sc, sh, LN_EPS)
        check_offtie(got, scaled64(y64, ref.scale), what)
        check_fused_state(st, ref, y64, what)
        if mod == "subnormal" and rows == "plain":
            sub = ((got & 0x7F) > 0) & ((got & 0x7F) < 8)
            assert sub.float().mean() > 0.25, what
    return check


def _ln_prior(pos, level):
    def check(be):
        what = f"ln prior {pos} {level}"
        x, sc, sh = ln_prior_case(pos)
        y64 = C.layer_norm_mod_f64(x, sc, sh, LN_EPS)
        rowmax = y64.abs().amax(-1).flatten().sort().values
        top = rowmax[-1].item()
        prior = {"below": 0.5 * rowmax[0].item(),
                 "between": 0.5 * (rowmax[-2].item() + top),
                 "above": 2.0 * top}[level]
        st = DelayedScale(plain_qscale(y64), amax=prior)
        ref = st.clone()
        got = be.ln(x, sc, sh, st)
        check_offtie(got, scaled64(y64, ref.scale), what)
        check_fused_state(st, ref, y64, what)
    return check


def ln_nan_row(be):
    """A NaN in one row: that row is NaN bytes, the others and the amax are
    untouched by it."""
    x, sc, sh, _ = ln_case((1, 3, 64), "plain", "plain", seed=5)
    x = x.clone()
    x[0, 1, 5] = math.nan
    y64 = C.layer_norm_mod_f64(x, sc, sh, LN_EPS)
    st = DelayedScale(plain_qscale(y64[0, ::2]))
    ref = st.clone()
    got = be.ln(x, sc, sh, st)
    assert is_nan_byte(got.view(3, 64)[1]).all(), "ln nan_row"
    check_offtie(got, scaled64(y64, ref.scale), "ln nan_row")
    check_fused_state(st, ref, y64, "ln nan_row")
    assert torch.isfinite(st.amax).all() and torch.isfinite(st.scale).all()


def _shape_id(shape):
    return "x".join(str(s) for s in shape)


CHECKS = {}
for _case in QUANT_INPUTS:
    for _s in SCALES:
        CHECKS[f"quant {_case} scale={_s}"] = _quant_bytes(_case, _s)
CHECKS["quant sequence"] = quant_sequence
for _pos in PRIOR_PEAKS:
    for _level in PRIOR_LEVELS:
        CHECKS[f"quant prior {_pos} {_level}"] = _quant_prior(_pos, _level)
CHECKS["quant one_slot"] = quant_one_slot
CHECKS["quant aliased"] = quant_aliased
CHECKS["quant floor"] = quant_floor
CHECKS["quant nonfinite"] = quant_nonfinite
CHECKS["large quant"] = _large("quant")
CHECKS["large gelu"] = _large("gelu")
for _s in GELU_SCALES:
    CHECKS[f"gelu all_finite_bf16 scale={_s}"] = _gelu_all(_s)
CHECKS["gelu nan_inf"] = gelu_nan_inf
for _shape, _rows, _mod in LN_CASES:
    CHECKS[f"ln {_shape_id(_shape)} {_rows} {_mod}"] = _ln(_shape, _rows, _mod)
for _pos in ("first", "last"):
    for _level in PRIOR_LEVELS:
        CHECKS[f"ln prior {_pos} {_level}"] = _ln_prior(_pos, _level)
CHECKS["ln nan_row"] = ln_nan_row


def offtie_cases():
    """(name, v64, v32) of every case judged by the off-tie criterion: the
    exact scaled values and the faithful emulation's, for the 5% cap and
    the emulation's distance from the margin."""
    def both(y64, y32, q):
        return scaled64(y64, f32(q)), scaled64(y32.double(), f32(q))

    pat = large_pattern()
    yield ("large gelu",) + both(gelu_f64(pat), gelu_f32(pat), UNIT)
    x = all_finite_bf16()
    for s in GELU_SCALES:
        yield (f"gelu all_finite_bf16 scale={s}",) + both(
            gelu_f64(x), gelu_f32(x), SCALES[s])
    for shape, rows, mod in LN_CASES:
        x, sc, sh, q = ln_case(shape, rows, mod)
        yield (f"ln {_shape_id(shape)} {rows} {mod}",) + both(
            C.layer_norm_mod_f64(x, sc, sh, LN_EPS), ln_f32(x, sc, sh), q)
    for pos in ("first", "last"):
        x, sc, sh = ln_prior_case(pos)
        y64 = C.layer_norm_mod_f64(x, sc, sh, LN_EPS)
        yield (f"ln prior {pos}",) + both(y64, ln_f32(x, sc, sh),
                                          plain_qscale(y64))
