"""Cases, fp64 references and faulty emulations for the rotary, packing,
gating and timestep kernels: qk_norm_rope_, pack_joint_qkv, rope_apply,
gate_residual, gelu_tanh's large launches, timestep_embedding and
timestep_embed_mlp.

Shared by test_elementwise_cases_reference.py (CPU: the faithful emulation
passes every check, every named fault is rejected by a named check, and
ops.* on the CPU keeps the same contract) and test_gpu_elementwise_exact.py
(GPU: the native kernels through the same checks). Everything here is
CPU-only and deterministic; a backend (`Emulated`, or `OpsBackend` on the
CPU or on a GPU) takes CPU tensors and returns CPU tensors.

Why not randn, arange(S) tables and t = rand: a rope_freqs(arange(S)) table
at S <= 5 turns the upper third of the pairs by less than 0.01 rad, so any
fault there is below atol = 2e-2; unit-variance rows with weights near 1 do
not tell q's weight from k's; and rand * 1000 never leaves the +-256
revolutions for which the ISA defines the hardware sine and cosine, while
the callers pass 4000 and 14610 rad.

The criterion for 16-bit outputs is the distance from the fp64 value in
units of the output type's spacing at that value, at most 0.5 + SLACK, with
no absolute term; see SLACK below.
"""
import math

import torch

import fp8_cases as F8
import kernel_cases as C
from comfyui_parallelanything_amd.models.layers import rope_2d_table
from comfyui_parallelanything_amd.models.wan import rope_3d_table
from comfyui_parallelanything_amd.ops import reference as R

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES16 = {"bf16": BF16, "fp16": F16}
DTYPES = {"bf16": BF16, "fp16": F16, "fp32": F32}
PERIOD = F8.PERIOD
GRID = 4096 * 256                  # threads of a capped grid_1d launch
TOL_FP32 = (1e-5, 1e-5)            # test_scalar_rungs_fp32's

# --------------------------------------------------------------------------
# The 16-bit criterion.
#
# SLACK: what fp32 arithmetic in the kernels' operation order may differ
# from fp64 before the final rounding to 16 bits, in spacings of the output
# type. Measured on the CPU over every 16-bit case of this file
# (test_slack_is_twice_the_measured_worst), with the multiply-adds fused and
# unfused and the reciprocal square root one fp32 ulp up and down:
#     measured worst   0.1071 spacings (qk_norm_rope_, model_slice table,
#                      D = 64, fp16: an output that is the difference of two
#                      products 200 times its size, so the fp32 roundings
#                      of the products weigh 200-fold against its spacing;
#                      pack_joint_qkv 0.0865; bf16 stays below 0.01)
#     chosen           SLACK = 2 * 0.1071, rounded up to 0.22
# Twice the worst covers the two instructions whose last bit the emulation
# cannot know (v_rsq_f32, and fma against mul + add).
# --------------------------------------------------------------------------
SLACK_MEASURED = 0.1071
SLACK = 0.22


def spacing16(v64, dtype):
    """Distance between neighbouring values of `dtype` at |v| (fp64 in and
    out); the subnormal spacing below the smallest normal."""
    mant, emin = (7, -126) if dtype == BF16 else (10, -14)
    _, e = torch.frexp(v64.abs())
    e = (e.to(torch.float64) - 1).clamp(min=emin)
    e = torch.where(v64 == 0, torch.full_like(e, emin), e)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def error_in_spacings(got, v64, dtype):
    return ((got.double() - v64).abs() / spacing16(v64, dtype))


def check16(got, v64, dtype, what=""):
    """`got` (dtype) against the fp64 value: finite and within 0.5 + SLACK
    spacings everywhere."""
    assert got.dtype == dtype, f"{what}: {got.dtype}"
    assert got.shape == v64.shape, f"{what}: {tuple(got.shape)}"
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    e = error_in_spacings(got, v64, dtype)
    worst = e.max().item() if e.numel() else 0.0
    assert worst <= 0.5 + SLACK, (
        f"{what}: {worst:.4f} spacings from fp64 at "
        f"{int(e.flatten().argmax())} (limit {0.5 + SLACK:.4f})")


def check_out(got, v64, dtype, what=""):
    if dtype == F32:
        assert got.dtype == F32 and got.shape == v64.shape, what
        C.check(got, v64, *TOL_FP32, what=what)
    else:
        check16(got, v64, dtype, what)


def same_bits(got, want, what=""):
    """Bit equality through an integer view: NaN payloads and -0 count."""
    assert got.dtype == want.dtype and got.shape == want.shape, (
        f"{what}: {got.dtype} {tuple(got.shape)} against "
        f"{want.dtype} {tuple(want.shape)}")
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]
    bad = got.contiguous().view(it) != want.contiguous().view(it)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in bits, "
        f"first at {int(bad.flatten().nonzero()[0])}")


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _hash(*idx):
    """A deterministic integer hash of broadcastable int64 index tensors."""
    h = torch.zeros((), dtype=torch.int64)
    for k, i in enumerate(idx):
        h = (h ^ (i.to(torch.int64) + 0x9E3779B9 + k)) * 0x85EBCA6B
        h = (h ^ (h >> 13)) & 0x7FFFFFFF
    h = (h * 0xC2B2AE35) & 0x7FFFFFFF
    return h ^ (h >> 16)


# --------------------------------------------------------------------------
# Builders. A test of the reference file replaces one of these by the old
# inputs (OLD_BUILDERS) and must then fail.
# --------------------------------------------------------------------------

def spread(shape, dtype, seed):
    """Off randn: magnitudes log-uniform over 2^-3 .. 2^3, random signs."""
    g = _gen(seed)
    mag = torch.exp2(torch.rand(shape, generator=g) * 6 - 3)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(dtype)


def unit_rows(shape, dtype, seed=0):
    """[..., D] rows of index-coded powers of two whose mean square is
    exactly 1: groups of five hold one 2 and four 1/2 (4 + 4/4 = 5), the
    rest 1; the place of the 2 and every sign come from a hash of the
    element's index. With eps = 0 the RMS is exactly 1, so unit weights and
    a quarter-turn table give an exact signed permutation."""
    D = shape[-1]
    rows = math.prod(shape[:-1])
    r = torch.arange(rows)[:, None]
    d = torch.arange(D)[None, :]
    grp, pos = d // 5, d % 5
    full = grp < D // 5
    two = _hash(r, grp, torch.tensor(seed)) % 5
    mag = torch.where(full, torch.where(pos == two, 2.0, 0.5), 1.0)
    sign = (_hash(r, d, torch.tensor(seed + 1)) % 2) * 2.0 - 1.0
    return (mag * sign).reshape(shape).to(dtype)


def pow2_rows(shape, dtype, seed, lo=-1, hi=1):
    """+-2^e, e in lo..hi, by a hash of the flat index."""
    i = torch.arange(math.prod(shape))
    e = lo + _hash(i, torch.tensor(seed)) % (hi - lo + 1)
    sign = (_hash(i, torch.tensor(seed + 7)) % 2) * 2.0 - 1.0
    return (torch.exp2(e.double()) * sign).reshape(shape).to(dtype)


QUARTER = torch.tensor([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])


def quarter_table(S, pairs, seed=0):
    """[S, pairs, 2] fp32: every (s, pair) entry a quarter turn picked by a
    hash of (s, pair), so all pairs, the upper ones too, turn by at least
    90 degrees or visibly not at all, and no two rows of the table agree."""
    s = torch.arange(S)[:, None]
    p = torch.arange(pairs)[None, :]
    return QUARTER[_hash(s, p, torch.tensor(seed)) % 4].contiguous()


AXES_DIM = {2: (2,), 6: (2, 2, 2), 40: (8, 16, 16), 64: (16, 24, 24),
            128: (16, 56, 56), 256: (32, 112, 112)}
TXT_LEN, GRID_HW = 7, (3, 4)           # rope_2d_table: 7 + 3 * 4 = 19 rows


def model_table(D, skip=0):
    """rope_2d_table as MMDiT builds it (the models' axes_dim at D = 128),
    from row `skip` on: skip = T is the pe[T:] slice the models pass."""
    axes = AXES_DIM[D]
    if len(axes) == 1:
        axes = (D, 0, 0)
    pe = rope_2d_table(*GRID_HW, axes, 10000.0, None, TXT_LEN)
    return pe[skip:]


def wan_table(D, f=2, h=2, w=3):
    axes = AXES_DIM[D]
    if len(axes) == 1:
        axes = (D, 0, 0)
    return rope_3d_table(f, h, w, axes, 10000.0, None)


def ts_arguments():
    """The values t * time_factor takes, as (t fp32 [B], time_factor)
    pairs: inside the hardware's 256 revolutions (1608 rad), at its edge
    (1600, 1616), FLUX's default guidance (4000), the k-diffusion sigma_max
    (14610), a negative one; and the same set with time_factor = 1."""
    args = [0.0, 1e-3, 1.0, 999.0, 1000.0, 1600.0, 1616.0, 4000.0, 14610.0,
            -4000.0]
    a = torch.tensor(args, dtype=F32)
    return ((a / 1000.0, 1000.0), (a.clone(), 1.0))


BUILDERS = {"spread": spread, "unit_rows": unit_rows, "pow2_rows": pow2_rows,
            "quarter_table": quarter_table, "model_table": model_table,
            "wan_table": wan_table, "ts_arguments": ts_arguments}


def _old_rows(shape, dtype, seed=0, *a, **k):
    return torch.randn(shape, generator=_gen(seed)).to(dtype)


def _old_table(S, pairs, seed=0):
    return R.rope_freqs(torch.arange(S), 2 * pairs)


def _old_model_table(D, skip=0, **k):
    return R.rope_freqs(torch.arange(TXT_LEN + GRID_HW[0] * GRID_HW[1]), D)[
        skip:]


def _old_wan_table(D, f=2, h=2, w=3):
    return R.rope_freqs(torch.arange(f * h * w), D)


def _old_ts_arguments():
    return ((torch.rand(10, generator=_gen(3)), 1000.0),
            (torch.rand(10, generator=_gen(4)), 1.0))


# what each builder stood for in the earlier tests
OLD_BUILDERS = {"spread": _old_rows, "unit_rows": _old_rows,
                "pow2_rows": _old_rows, "quarter_table": _old_table,
                "model_table": _old_model_table, "wan_table": _old_wan_table,
                "ts_arguments": _old_ts_arguments}


def build(name, *a, **k):
    """Every case draws its inputs through here, so that a test can swap a
    builder."""
    return BUILDERS[name](*a, **k)


# --------------------------------------------------------------------------
# fp32 arithmetic in the kernels' order
# --------------------------------------------------------------------------

def _madd(a, b, c, fused):
    """a * b + c in fp32: one rounding (fma) or two."""
    if fused:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _rot(a0, a1, c, s, fused):
    """(a0 c - a1 s, a0 s + a1 c) as rms_rope_pair and rope_apply_kernel
    write it: the compiler may contract either product into the sum."""
    return (_madd(a0, c, -(a1 * s), fused), _madd(a0, s, a1 * c, fused))


def _ulp_shift(x, n):
    return (x.view(torch.int32) + n).view(F32) if n else x


def _wave_sum(v):
    """wave_reduce_sum: the xor-shuffle tree over 64 lanes, [..., 64]."""
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    return v[..., 0]


def rms_rope_rows(x, w, c, s, eps, fused=True, rsq_ulp=0):
    """rms_rope_pair over rows: x [N, D] (16-bit), w [N, D] or [D], c / s
    [N, D/2] fp32 -> [N, D] fp32, before the final rounding."""
    N, D = x.shape
    a = x.float().view(N, D // 2, 2)
    a0, a1 = a[..., 0], a[..., 1]
    sq = torch.zeros(N, 64)
    sq[:, :D // 2] = _madd(a0, a0, a1 * a1, fused)
    ss = _wave_sum(sq)
    rr = _ulp_shift(1.0 / torch.sqrt(ss / D + torch.tensor(eps, dtype=F32)),
                    rsq_ulp)[:, None]
    wf = w.float().expand(N, D).reshape(N, D // 2, 2)
    a0 = a0 * rr * wf[..., 0]
    a1 = a1 * rr * wf[..., 1]
    o0, o1 = _rot(a0, a1, c, s, fused)
    return torch.stack([o0, o1], -1).view(N, D)


def _flat(t):
    """The whole storage behind a view, as a flat tensor of its dtype."""
    n = t.untyped_storage().nbytes() // t.element_size()
    return torch.as_strided(t, (n,), (1,), 0)


# ---- qk_norm_rope_ ---------------------------------------------------------

QK_FAULTS = ("cs_row_next", "cs_row_prev", "cs_by_row", "pair_shifted",
             "upper_unrotated", "direction_flipped", "w0_w1_swapped",
             "wq_for_k", "batch_stride_ignored", "tail_rows_stored",
             "dead_lanes_stored")


def emulate_qk_norm_rope_(q, k, wq, wk, cs, eps, fault=None, fused=True,
                          rsq_ulp=0):
    """qk_norm_rope_kernel on CPU views, in place, by its own address
    arithmetic: row -> (b, s, h) -> base + b * bs + s * ss + h * hs +
    2 * lane, four rows per wave with the tail rows clamped."""
    B, S, H, D = q.shape
    pairs = D // 2
    n_rows = B * S * H
    csf = cs.float().contiguous()
    lane = torch.arange(pairs)

    def one(x, w, rows, stored):
        """Loads rows `rows` of x, returns (addresses, values) of what the
        wave stores; `stored` selects the rows it does store."""
        rr = rows.clamp(max=n_rows - 1)
        b, sh = rr // (S * H), rr % (S * H)
        sj, h = sh // H, sh % H
        bs, ss, hs, _ = x.stride()
        if fault == "batch_stride_ignored":
            bs = 0
        base = x.storage_offset() + b * bs + sj * ss + h * hs
        flat = _flat(x)
        addr = base[:, None] + 2 * lane[None, :]
        xr = torch.stack([flat[addr], flat[addr + 1]], -1).view(-1, D)
        cj = sj
        if fault == "cs_row_next":
            cj = (sj + 1) % S
        if fault == "cs_row_prev":
            cj = (sj - 1) % S
        if fault == "cs_by_row":
            cj = rr % S
        pj = (lane + 1) % pairs if fault == "pair_shifted" else lane
        c, s = csf[cj][:, pj, 0], csf[cj][:, pj, 1]
        if fault == "upper_unrotated":
            c = torch.where(lane >= (pairs + 1) // 2, torch.ones(()), c)
            s = torch.where(lane >= (pairs + 1) // 2, torch.zeros(()), s)
        if fault == "direction_flipped":
            s = -s
        wv = w.float()
        if fault == "w0_w1_swapped":
            wv = wv.view(pairs, 2).flip(1).reshape(D)
        out = rms_rope_rows(xr, wv, c, s, eps, fused, rsq_ulp).to(x.dtype)
        out = out.view(-1, pairs, 2)
        return (addr[stored], out[stored], base[stored], xr[stored])

    def run(x, w):
        flat = _flat(x)
        real = torch.arange(n_rows)
        addr, out, base, xr = one(x, w, real, real >= 0)
        if fault == "dead_lanes_stored" and pairs < 64:
            # lanes >= pairs computed from the clamped lane 0 and stored at
            # their own offset, past the row
            dead = torch.arange(pairs, 64)
            da = base[:, None] + 2 * dead[None, :]
            ok = da + 1 < flat.numel()
            for j in (0, 1):
                v = out[:, :1, j].expand(-1, dead.numel())
                flat[(da + j)[ok]] = v[ok]
        flat[addr] = out[..., 0]
        flat[addr + 1] = out[..., 1]
        if fault == "tail_rows_stored":
            # the clamped rows of the last wave, loaded again and stored
            for row in range(n_rows, -(-n_rows // 4) * 4):
                r = torch.tensor([row])
                a, o, _, _ = one(x, w, r, r >= 0)
                flat[a] = o[..., 0]
                flat[a + 1] = o[..., 1]

    run(q, wq)
    run(k, wq if fault == "wq_for_k" else wk)


QK_SHAPE = (3, 5, 3)               # B, S, H: 45 rows, the last wave holds one
QK_DIMS = (2, 40, 64, 128)
QK_LAYOUTS = ("fused", "permuted", "sliced")
NAN16 = {BF16: 0x7FC1, F16: 0x7E01}


def _guarded(shape, dtype):
    """A buffer of NaN guards (a payload no arithmetic produces)."""
    pat = NAN16[dtype]
    pat = pat - 0x10000 if pat >= 0x8000 else pat
    return torch.full(shape, pat, dtype=torch.int16).view(dtype)


def _distinct(shape, dtype):
    """All-distinct 16-bit patterns (NaN payloads, -0, infinities among
    them when there are enough elements)."""
    n = math.prod(shape)
    i = (torch.arange(n) * 40503 + 12345) % 65536     # 40503 is odd
    return (i - 65536 * (i >= 32768)).to(torch.int16).view(dtype).reshape(
        shape)


def qk_layout(layout, D, dtype):
    """(bufs, views): freshly guarded base buffers and views(bufs) -> (q,
    k), both [B, S, H, D] views into them."""
    B, S, H = QK_SHAPE
    if layout == "fused":
        buf = _guarded((B, S, 3, H, D), dtype)
        buf[:, :, 2] = _distinct((B, S, H, D), dtype)
        return [buf], lambda b: (b[0][:, :, 0], b[0][:, :, 1])
    if layout == "permuted":       # k's head stride exceeds its sequence's
        return ([_guarded((B, S, H, D), dtype),
                 _guarded((B, H, S, D), dtype)],
                lambda b: (b[0], b[1].permute(0, 2, 1, 3)))
    return ([_guarded((B, S, H, D + 16), dtype),
             _guarded((B, S, H, D + 16), dtype)],
            lambda b: (b[0][..., 8:8 + D], b[1][..., 8:8 + D]))


def view_masks(bufs, views):
    marks = [torch.zeros(b.shape, dtype=torch.bool) for b in bufs]
    for v in views(marks):
        v.fill_(True)
    return marks


def qk_tables(D):
    """name -> cs as the caller passes it, [S, D/2, 2] for S = 5."""
    S = QK_SHAPE[1]
    pairs = D // 2
    wide = torch.zeros(S, pairs + 3, 4)
    wide[:, 1:1 + pairs, 1:3] = build("quarter_table", S, pairs, 5)
    return {
        "quarter": build("quarter_table", S, pairs),
        "model": build("model_table", D)[TXT_LEN - 2:TXT_LEN + 3],
        "model_slice": build("model_table", D, TXT_LEN)[:S],
        "wan": build("wan_table", D)[1:1 + S],
        "fp64": build("model_table", D)[:S].double(),
        "bf16": build("model_table", D)[-S:].to(BF16),
        "strided": wide[:, 1:1 + pairs, 1:3],        # non-contiguous
    }


QK_TABLES = ("quarter", "model", "model_slice", "wan", "fp64", "bf16",
             "strided")
QK_EPS = 1e-6


def _weights(D, dtype, seed):
    """Off 1: 0.5 .. 2, wq and wk far apart, w0 != w1 in every pair."""
    g = _gen(seed)
    return (torch.exp2(torch.rand(D, generator=g) * 2 - 1)
            * (1 + (torch.arange(D) % 2))).to(dtype) / 1.5


def qk_case(layout, table, D, dtype):
    bufs, views = qk_layout(layout, D, dtype)
    q, k = views(bufs)
    exact = table in ("quarter", "strided")
    cs = qk_tables(D)[table]
    if exact:
        q.copy_(build("unit_rows", q.shape, dtype, 1))
        k.copy_(build("unit_rows", k.shape, dtype, 2))
        wq = torch.ones(D, dtype=dtype)
        wk = torch.ones(D, dtype=dtype)
        eps = 0.0
    else:
        q.copy_(build("spread", q.shape, dtype, 11 + D))
        k.copy_(build("spread", k.shape, dtype, 12 + D))
        wq, wk = _weights(D, dtype, 3), _weights(D, dtype, 4).flip(0) * 1.25
        wk = wk.to(dtype)
        eps = QK_EPS
    return bufs, views, wq, wk, cs, eps, exact


def _qk_check(layout, table, D, dname):
    dtype = DTYPES16[dname]

    def check(be):
        what = f"qk {layout} {table} D={D} {dname}"
        bufs, views, wq, wk, cs, eps, exact = qk_case(layout, table, D, dtype)
        q0, k0 = (v.clone() for v in views(bufs))
        csr = cs.float() if cs.dtype != torch.float64 else cs.float()
        ref_q = C.qk_norm_rope_f64(q0, wq, csr, eps)
        ref_k = C.qk_norm_rope_f64(k0, wk, csr, eps)
        before = [b.clone() for b in bufs]
        after = be.qk_norm_rope_(bufs, views, wq, wk, cs, eps)
        # everything outside the views is bit for bit what it was
        for i, m in enumerate(view_masks(bufs, views)):
            a16 = after[i].view(torch.int16)
            b16 = before[i].view(torch.int16)
            bad = (a16 != b16) & ~m
            assert not bad.any(), (
                f"{what}: {int(bad.sum())} elements outside the views "
                f"changed in buffer {i}")
        q1, k1 = views(after)
        if exact:
            same_bits(q1.contiguous(), ref_q.to(dtype), what + " q")
            same_bits(k1.contiguous(), ref_k.to(dtype), what + " k")
        check16(q1.contiguous(), ref_q, dtype, what + " q")
        check16(k1.contiguous(), ref_k, dtype, what + " k")
    return check


# ---- pack_joint_qkv --------------------------------------------------------

PACK_FAULTS = ("img_cs_local", "boundary_late", "boundary_early",
               "txt_weights_on_img", "qkv_stride_swapped", "local_order")
PACK_DIMS = (40, 128)
PACK_SHAPES = ((3, 2, 3, 3), (2, 0, 3, 3), (2, 3, 0, 3))    # B, T, Si, H
PACK_LAYOUTS = ("img_sliced", "txt_sliced")
PACK_ALL16 = (4, 16, 16, 4)        # 512 rows of D = 128: 65536 elements of v


def emulate_pack_joint_qkv(txt, img, wq_t, wk_t, wq_i, wk_i, cs, eps,
                           fault=None, fused=True, rsq_ulp=0):
    """pack_joint_qkv_kernel: joint row -> (b, sj, h), stream by sj < T,
    source address from that stream's strides, output row contiguous."""
    B, T, _, H, D = txt.shape
    Si = img.shape[1]
    S = T + Si
    pairs = D // 2
    n_rows = B * S * H
    dtype = txt.dtype
    outs = [torch.zeros(B, S, H, D, dtype=dtype) for _ in range(3)]
    if n_rows == 0:
        return outs
    csf = cs.float().contiguous()
    rows = torch.arange(n_rows)
    b, sh = rows // (S * H), rows % (S * H)
    sj, h = sh // H, sh % H
    Tb = T + (fault == "boundary_late") - (fault == "boundary_early")
    is_txt = sj < Tb
    lane = torch.arange(pairs)

    def src(t, s_local, qkv, other):
        """Flat addresses [rows, D] into t's storage (wrapped into it where
        a fault walks out of the tensor)."""
        bs, ss, qs, hs, _ = t.stride()
        if fault == "qkv_stride_swapped":
            qs = other.stride(2)
        a = (t.storage_offset() + b * bs + s_local * ss + h * hs + qkv * qs)
        a = a[:, None] + torch.arange(D)[None, :]
        n = _flat(t).numel()
        return _flat(t)[a % n] if n else torch.zeros(n_rows, D, dtype=dtype)

    cj = torch.where(is_txt, sj, sj - T) if fault == "img_cs_local" else sj
    c, s = csf[cj][:, lane, 0], csf[cj][:, lane, 1]
    if fault == "local_order":       # img rows first, then txt
        so = torch.where(is_txt, sj + Si, sj - T)
    else:
        so = sj
    for qkv, (w_t, w_i) in enumerate(((wq_t, wq_i), (wk_t, wk_i), (None,) * 2)):
        x = torch.where(is_txt[:, None], src(txt, sj, qkv, img),
                        src(img, sj - T, qkv, txt))
        if qkv == 2:
            val = x
        else:
            if fault == "txt_weights_on_img":
                w_i = w_t
            w = torch.where(is_txt[:, None], w_t.float()[None],
                            w_i.float()[None])
            val = rms_rope_rows(x, w, c, s, eps, fused, rsq_ulp).to(dtype)
        outs[qkv][b, so, h] = val
    return outs


def pack_layout(shape, layout, D, dtype):
    """(txt, img) [B, S, 3, H, D]: one contiguous, the other a [..., 8:8+D]
    slice of a NaN-guarded buffer with a last dimension of D + 16."""
    B, T, Si, H = shape
    plain = lambda S: _guarded((B, S, 3, H, D), dtype)
    sliced = lambda S: _guarded((B, S, 3, H, D + 16), dtype)[..., 8:8 + D]
    if layout == "img_sliced":
        return plain(T), sliced(Si)
    return sliced(T), plain(Si)


def pack_case(shape, layout, table, D, dtype):
    B, T, Si, H = shape
    txt, img = pack_layout(shape, layout, D, dtype)
    S = T + Si
    exact = table == "quarter"
    if exact:
        cs = build("quarter_table", S, D // 2, 9)
        txt[:, :, :2] = build("unit_rows", (B, T, 2, H, D), dtype, 3)
        img[:, :, :2] = build("unit_rows", (B, Si, 2, H, D), dtype, 4)
        sgn = (torch.arange(D) % 3 == 0) * -2.0 + 1.0
        ws = [(sgn * m).to(dtype) for m in (1.0, 2.0, 0.5, 4.0)]
        ws[1] = ws[1].flip(0).contiguous()
        eps = 0.0
    else:
        cs = build("model_table", D)[TXT_LEN - T:TXT_LEN + Si]
        txt[:, :, :2] = build("spread", (B, T, 2, H, D), dtype, 21 + D)
        img[:, :, :2] = build("spread", (B, Si, 2, H, D), dtype, 22 + D)
        ws = [_weights(D, dtype, 30 + i) * (1 + 0.5 * i) for i in range(4)]
        ws = [w.to(dtype) for w in ws]
        eps = QK_EPS
    # v: distinct 16-bit patterns, all 65536 of them at PACK_ALL16
    v = _distinct((B, S, H, D), dtype)
    txt[:, :, 2] = v[:, :T]
    img[:, :, 2] = v[:, T:]
    return txt, img, ws, cs, eps, exact, v


def pack_ref(txt, img, ws, cs, eps):
    q = torch.cat([C.qk_norm_rope_f64(txt[:, :, 0], ws[0], cs[:txt.shape[1]], eps),
                   C.qk_norm_rope_f64(img[:, :, 0], ws[2], cs[txt.shape[1]:], eps)], 1)
    k = torch.cat([C.qk_norm_rope_f64(txt[:, :, 1], ws[1], cs[:txt.shape[1]], eps),
                   C.qk_norm_rope_f64(img[:, :, 1], ws[3], cs[txt.shape[1]:], eps)], 1)
    return q, k


def _pack_check(shape, layout, table, D, dname):
    dtype = DTYPES16[dname]

    def check(be):
        B, T, Si, H = shape
        what = f"pack {shape} {layout} {table} D={D} {dname}"
        txt, img, ws, cs, eps, exact, v = pack_case(shape, layout, table, D,
                                                    dtype)
        t0, i0 = txt.clone(), img.clone()
        oq, ok, ov = be.pack_joint_qkv(txt, img, *ws, cs, eps)
        for o in (oq, ok, ov):
            assert o.shape == (B, T + Si, H, D) and o.is_contiguous(), what
        same_bits(txt.contiguous(), t0, what + " txt read only")
        same_bits(img.contiguous(), i0, what + " img read only")
        rq, rk = pack_ref(t0, i0, ws, cs.float(), eps)
        same_bits(ov, v, what + " v")
        if exact:
            same_bits(oq, rq.to(dtype), what + " q")
            same_bits(ok, rk.to(dtype), what + " k")
        check16(oq, rq, dtype, what + " q")
        check16(ok, rk, dtype, what + " k")
        if T == 0 or Si == 0:
            # one stream alone is qk_norm_rope_ of that stream
            one = img if T == 0 else txt
            w = ws[2:] if T == 0 else ws[:2]
            bufs = [one.clone()]
            views = lambda b: (b[0][:, :, 0], b[0][:, :, 1])
            after = be.qk_norm_rope_(bufs, views, w[0], w[1], cs, eps)
            sq, sk = views(after)
            same_bits(oq, sq.contiguous(), what + " q single stream")
            same_bits(ok, sk.contiguous(), what + " k single stream")
    return check


# ---- rope_apply ------------------------------------------------------------

ROPE_FAULTS = ("s_without_mod", "h_ignored", "last_trip_skipped",
               "second_trip_reads_first")
ROPE_SHAPE = (2, 3, 5)             # B, H, S
ROPE_DIMS = (2, 6, 64)
ROPE_LARGE = (1, 1, 8203, 256)     # 1 049 984 pairs > 4096 * 256


def emulate_rope_apply(x, cs, fault=None, fused=True):
    """rope_apply_kernel: pair i of the flat tensor, pair = i % Dh, s =
    (i / Dh) % S; thread g takes pairs g, g + stride, ..."""
    B, H, S, D = x.shape
    Dh = D // 2
    n = x.numel() // 2
    stride = min((n + 255) // 256, 4096) * 256
    csf = cs.float().contiguous().view(S * Dh, 2)
    i = torch.arange(n)
    pair = i % Dh
    s = (i // Dh) % S
    if fault == "s_without_mod":
        s = (i // Dh).clamp(max=S - 1)
    if fault == "h_ignored":           # rows taken as [B, S], not [B, H, S]
        s = (i // (Dh * H)) % S
    src = i
    if fault == "second_trip_reads_first":
        src = torch.where(i >= stride, i - stride, i)
    xf = x.float().reshape(n, 2)[src]
    c, sn = csf[s * Dh + pair, 0], csf[s * Dh + pair, 1]
    o0, o1 = _rot(xf[:, 0], xf[:, 1], c, sn, fused)
    out = torch.stack([o0, o1], -1)
    if fault == "last_trip_skipped":
        out[(n - 1) // stride * stride:] = 0
    return out.reshape(x.shape), out.reshape(x.shape).to(x.dtype)


def rope_case(table, D, dtype):
    B, H, S = ROPE_SHAPE
    if table == "quarter":
        x = build("pow2_rows", (B, H, S, D), dtype, 5, -2, 2)
        cs = build("quarter_table", S, D // 2, 2)
    else:
        x = build("spread", (B, H, S, D), dtype, 40 + D)
        cs = build("model_table", D)[TXT_LEN - 2:TXT_LEN + 3]
    return x, cs


def rope_large_case(dtype):
    """Pairs with a period of PERIOD (odd, so coprime to the 2^20 pairs of
    one trip): what the second trip must read differs from the first's."""
    B, H, S, D = ROPE_LARGE
    n = B * H * S * D // 2
    pat = build("pow2_rows", (PERIOD, 2), dtype, 6, -2, 2)
    x = pat[torch.arange(n) % PERIOD].reshape(ROPE_LARGE)
    return x, build("quarter_table", S, D // 2, 3)


def _rope_ref(x, cs):
    """rope_f64 takes [B, S, H, D]."""
    return C.rope_f64(x.permute(0, 2, 1, 3), cs).permute(0, 2, 1, 3)


def _rope_check(table, D, dname):
    dtype = DTYPES[dname]

    def check(be):
        what = f"rope {table} D={D} {dname}"
        if table == "large":
            x, cs = rope_large_case(dtype)
        else:
            x, cs = rope_case(table, D, dtype)
        x0 = x.clone()
        out = be.rope_apply(x, cs)
        same_bits(x, x0, what + " input read only")
        ref = _rope_ref(x0, cs)
        if table != "model":
            same_bits(out, ref.to(dtype), what)
        check_out(out, ref, dtype, what)
    return check


# ---- gate_residual ---------------------------------------------------------

GATE_FAULTS = ("b_from_wrong_S", "d_wrong_modulus", "gate_row_0",
               "last_vector_skipped", "last_trip_skipped")
GATE_SHAPES = {"vec": (3, 5, 24), "scalar": (3, 5, 20),
               "large_vec": (1, 4097, 2048), "large_scalar": (1, 52433, 20)}


def emulate_gate_residual(res, gate, x, fault=None):
    """Both kernels: flat item i (a vector of 8 where D % 8 == 0 in a
    16-bit type, else one element), d = i % D', b = i / (S D')."""
    B, S, D = x.shape
    vec = 8 if (x.dtype != F32 and D % 8 == 0) else 1
    Dv = D // vec
    n = x.numel() // vec
    stride = min((n + 255) // 256, 4096) * 256
    i = torch.arange(n)
    d = i % (Dv + 1 if fault == "d_wrong_modulus" else Dv)
    b = i // ((S + 1 if fault == "b_from_wrong_S" else S) * Dv)
    if fault == "gate_row_0":
        b = torch.zeros_like(b)
    g = gate.contiguous().float().view(B * Dv, vec)[(b * Dv + d) % (B * Dv)]
    out = (res.float().reshape(n, vec) + g * x.float().reshape(n, vec))
    if fault == "last_vector_skipped":
        out[-1] = 0
    if fault == "last_trip_skipped":
        out[(n - 1) // stride * stride:] = 0
    return out.reshape(x.shape).to(x.dtype)


def gate_case(kind, dtype, strided_gate=False):
    """Powers of two with exponents close enough for an exact result in
    every type: x, res in 2^-1..2^1, the gate 2^0..2^2 and different in
    every batch row and column."""
    B, S, D = GATE_SHAPES[kind]
    x = build("pow2_rows", (B, S, D), dtype, 50)
    res = build("pow2_rows", (B, S, D), dtype, 51)
    gate = build("pow2_rows", (B, 6, D), dtype, 52, 0, 2)
    if strided_gate:               # WanBlock: unbind(1) of a [B, 6, D] tensor
        return res, gate.unbind(1)[4], x
    return res, gate[:, 1].contiguous(), x


def _gate_check(kind, dname, strided_gate=False):
    dtype = DTYPES[dname]

    def check(be):
        what = f"gate {kind} {dname}" + (" unbind" if strided_gate else "")
        res, gate, x = gate_case(kind, dtype, strided_gate)
        assert gate.is_contiguous() != strided_gate
        out = be.gate_residual(res, gate, x)
        ref = res.double() + gate.double()[:, None] * x.double()
        same_bits(out, ref.to(dtype), what)
    return check


# ---- gelu_tanh: large launches ----------------------------------------------

GELU_LARGE_VECS = GRID + 4097      # a partial second trip


def gelu_large_case(kind, dtype):
    """(x, view): x a [rows, w] tensor whose vectors of 8 repeat with period
    PERIOD and hold the special values of gelu_values; `strided` is the
    left half of a buffer twice as wide."""
    vals = C.gelu_values(dtype)
    pat = build("spread", (PERIOD, 8), dtype, 60)
    pat[:len(vals) // 8] = vals.view(-1, 8)
    w8 = 256
    rows = -(-GELU_LARGE_VECS // w8)
    x = pat[torch.arange(rows * w8) % PERIOD].reshape(rows, w8 * 8)
    if kind == "strided":
        wide = torch.cat([x, -x], 1)
        return wide[:, :w8 * 8]
    return x


def _gelu_check(kind, dname):
    dtype = DTYPES16[dname]

    def check(be):
        what = f"gelu large {kind} {dname}"
        x = gelu_large_case(kind, dtype)
        assert x.is_contiguous() == (kind == "vector")
        out = be.gelu_tanh(x)
        assert out.shape == x.shape and out.dtype == dtype, what
        ref = torch.nn.functional.gelu(x.float(), approximate="tanh")
        C.check(out, ref, *C.TOL_GELU, what=what, equal_nan=True)
        # and no vector holds another vector's result
        first = out.reshape(-1, 8)[:PERIOD]
        idx = torch.arange(out.numel() // 8) % PERIOD
        same_bits(out.reshape(-1, 8), first[idx], what + " period")
    return check


# ---- timestep_embedding ----------------------------------------------------

TS_FAULTS = ("no_range_reduction", "argument_clamped", "halves_swapped",
             "half_from_dim", "odd_column_unwritten")
TS_DIMS = (1, 2, 3, 256, 320)
TS_PERIODS = (1e4, 100.0)
TS_LARGE = (1025, 512)             # B * dim / 2 / 256 = 1025 blocks > 1024
REV256 = 256 * 2 * math.pi         # 1608.5 rad

# --------------------------------------------------------------------------
# The bound on an fp32 timestep embedding: |out - fp64| <= TS_A + TS_B *
# |arg| * 2^-24, arg = t * time_factor * freq_j evaluated in fp64 on the
# fp32 t. The argument carries fp32 roundings (t * time_factor, the
# frequency's exponent, the product) that grow with it; the cos / sin itself
# adds a constant.
# Measured for reference.timestep_embedding (fp32 torch on the CPU) against
# fp64 over ts_arguments() x TS_DIMS x TS_PERIODS and the large launch
# (test_ts_bound_is_four_times_the_measured_one):
#     a: 3.73e-8 (the worst error where |arg| <= 1/16, where the
#        argument's own error is below a tenth of it)
#     b: 9.19 (the worst of (error - a) / (|arg| 2^-24) beyond: the
#        exponent -ln(P) j / half reaches 9.2, where half an fp32 ulp of it
#        is 8 * 2^-24 relative to the frequency)
# The kernel is allowed four times each: its frequency comes from the fast
# exp and log, a few ulps worse than torch's.
#     TS_A = 1.5e-7    TS_B = 36.8
# At |arg| = 14610 that is 0.032: fp32 cannot place such an argument within
# a revolution any better, and a missing range reduction is off by O(1).
# --------------------------------------------------------------------------
TS_A_MEASURED, TS_B_MEASURED = 3.73e-8, 9.19
TS_A, TS_B = 1.5e-7, 36.8
TS_SMALL = 1.0 / 16   # |arg| up to here measures a; beyond, b


def ts_f64(t, dim, max_period, time_factor):
    """(embedding, |argument|) in fp64 on the fp32 t, [B, dim] each; the
    odd column is 0 with argument 0."""
    half = dim // 2
    freq = torch.exp(-math.log(max_period)
                     * torch.arange(half, dtype=torch.float64) / max(half, 1))
    arg = t.float().double()[:, None] * time_factor * freq[None]
    emb = torch.cat([arg.cos(), arg.sin()], 1)
    mag = torch.cat([arg.abs(), arg.abs()], 1)
    if dim % 2:
        z = torch.zeros(len(t), 1, dtype=torch.float64)
        emb, mag = torch.cat([emb, z], 1), torch.cat([mag, z], 1)
    return emb, mag


def ts_bound(mag, a=None, b=None):
    a = TS_A if a is None else a
    b = TS_B if b is None else b
    return a + b * mag * 2.0 ** -24


def emulate_timestep_embedding(t, dim, max_period, time_factor, fault=None):
    """timestep_embedding_kernel in fp32 torch: freq = exp(-log(P) * j /
    half), arg = t * time_factor * freq, cos | sin halves."""
    half = dim // 2
    B = len(t)
    out = torch.full((B, dim), 7.0)            # "uninitialised"
    j = torch.arange(half, dtype=F32)
    denom = float(dim if fault == "half_from_dim" else max(half, 1))
    lg = torch.tensor(-math.log(max_period), dtype=F32)
    freq = torch.exp(lg * j / denom)
    arg = t.float()[:, None] * torch.tensor(time_factor, dtype=F32) * freq
    if fault == "argument_clamped":
        arg = arg.clamp(-REV256, REV256)
    c, s = torch.cos(arg), torch.sin(arg)
    if fault == "no_range_reduction":
        c = torch.where(arg.abs() > REV256, torch.ones(()), c)
        s = torch.where(arg.abs() > REV256, torch.zeros(()), s)
    if fault == "halves_swapped":
        c, s = s, c
    out[:, :half] = c
    out[:, half:2 * half] = s
    if dim % 2 and fault != "odd_column_unwritten":
        out[:, -1] = 0
    if half == 0 and fault != "odd_column_unwritten":
        out.zero_()
    return out


def check_ts(out, t, dim, max_period, time_factor, what=""):
    emb, mag = ts_f64(t, dim, max_period, time_factor)
    assert out.dtype == F32 and out.shape == emb.shape, what
    assert torch.isfinite(out).all(), f"{what}: non-finite"
    over = (out.double() - emb).abs() - ts_bound(mag)
    assert (over <= 0).all(), (
        f"{what}: {int((over > 0).sum())} of {over.numel()} outside the "
        f"bound, worst by {over.max().item():.3e} at "
        f"{int(over.flatten().argmax())}")
    if dim % 2:
        assert (out[:, -1] == 0).all(), f"{what}: odd column not zero"


def _ts_check(dim, max_period):
    def check(be):
        for t, tf in build("ts_arguments"):
            what = f"ts dim={dim} P={max_period:g} tf={tf:g}"
            check_ts(be.timestep_embedding(t, dim, max_period, tf), t, dim,
                     max_period, tf, what)
    return check


def ts_large_case():
    B, dim = TS_LARGE
    base = torch.cat([a * f for a, f in build("ts_arguments")])
    return base[torch.arange(B) % len(base)] + torch.arange(B) * 0.25, dim


def ts_large(be):
    t, dim = ts_large_case()
    check_ts(be.timestep_embedding(t, dim, 1e4, 1.0), t, dim, 1e4, 1.0,
             "ts large")


# ---- timestep_embed_mlp ----------------------------------------------------

MLP_FAULTS = ("b_from_block", "halves_swapped", "tail_block_past_H",
              "lds_fill_stops_at_256")
MLP_B, MLP_H = 3, 300              # two blocks per batch element, one partial
MLP_KS = (8, 256, 1024)


def emulate_ts_embed_mlp(t, w1, b1, max_period, time_factor, fault=None):
    """ts_embed_mlp_kernel: block (b, hblk) fills emb[K] in LDS (thread j,
    j + 256, ...), then thread o accumulates bias + sum_k emb[k] w[o, k] in
    k order and applies SiLU."""
    H, K = w1.shape
    B = len(t)
    half = K // 2
    hblocks = (H + 255) // 256
    emb_fault = fault if fault == "halves_swapped" else None
    out = torch.zeros(B * H + 256)
    wf = w1.float()
    for blk in reversed(range(B * hblocks)):
        b = blk // hblocks
        if fault == "b_from_block":
            b = min(blk, B - 1)
        emb = emulate_timestep_embedding(t[b:b + 1], K, max_period,
                                         time_factor, emb_fault)[0]
        if fault == "lds_fill_stops_at_256":
            emb[256:half] = 0
            emb[half + 256:] = 0
        o = (blk % hblocks) * 256 + torch.arange(256)
        if fault != "tail_block_past_H":
            o = o[o < H]
        acc = (b1.float()[o % H] if b1 is not None
               else torch.zeros(len(o)))
        wrows = wf[o % H]
        for k in range(K):             # fp32, in k order
            acc = acc + emb[k] * wrows[:, k]
        acc = acc / (1.0 + torch.exp(-acc))
        out[(blk // hblocks) * H + o] = acc
    return out[:B * H].view(B, H).to(BF16)


def mlp_case(K, bias):
    """One-hot bf16 rows: out[b, o] = silu(emb[b, k(o)] + bias[o]), with
    k(o) walking every quarter of K."""
    o = torch.arange(MLP_H)
    k = (o * (K // 4 + 1) + o // 4) % K
    w1 = torch.zeros(MLP_H, K)
    w1[o, k] = 1.0
    b1 = None
    if bias:
        b1 = (((o % 7) - 3) * 2.5).to(BF16)        # -7.5 .. 7.5
    return w1.to(BF16), b1, k


def _silu64(x):
    return x * torch.sigmoid(x)


def check_mlp(out, t, w1, b1, k, max_period, time_factor, what=""):
    """Against silu(fp64 embedding + bias): half a bf16 spacing plus SLACK,
    plus what the embedding's own bound lets through SiLU, whose slope is
    at most 1.1."""
    K = w1.shape[1]
    emb, mag = ts_f64(t, K, max_period, time_factor)
    pre = emb[:, k] + (b1.double()[None] if b1 is not None else 0.0)
    ref = _silu64(pre)
    assert out.dtype == BF16 and out.shape == ref.shape, what
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite"
    lim = ((0.5 + SLACK) * spacing16(ref, BF16)
           + 1.1 * ts_bound(mag[:, k]))
    over = (out.double() - ref).abs() - lim
    assert (over <= 0).all(), (
        f"{what}: {int((over > 0).sum())} of {over.numel()} outside the "
        f"bound, worst by {over.max().item():.3e} at "
        f"{int(over.flatten().argmax())}")


def _mlp_check(K, bias):
    def check(be):
        w1, b1, k = mlp_case(K, bias)
        for a, tf in build("ts_arguments"):
            # B = 3 per launch: the grid in consecutive threes, the last
            # launch wrapping round
            for i in range(0, len(a), MLP_B):
                t = a[(torch.arange(MLP_B) + i) % len(a)]
                what = f"mlp K={K} bias={bias} tf={tf:g} t={t.tolist()}"
                out = be.timestep_embed_mlp(t, w1, b1, 1e4, tf)
                check_mlp(out, t, w1, b1, k, 1e4, tf, what)
    return check


def mlp_composed(be):
    """The fused kernel against the composed path it replaces (embedding,
    bf16 cast, Linear, SiLU), as test_timestep_embed_mlp_matches_composed_
    path, on the argument grid and dense weights."""
    g = _gen(70)
    K, H = 256, MLP_H
    w1 = (torch.randn(H, K, generator=g) / 16).to(BF16)
    b1 = torch.randn(H, generator=g).to(BF16)
    for a, tf in build("ts_arguments"):
        t = a[[4, 7, 8]]
        fused = be.timestep_embed_mlp(t, w1, b1, 1e4, tf)
        emb = be.timestep_embedding(t, K, 1e4, tf).to(BF16)
        comp = torch.nn.functional.silu(
            emb.float() @ w1.float().t() + b1.float())
        C.check(fused, comp, 3e-2, 3e-2, what=f"mlp composed tf={tf:g}")


# --------------------------------------------------------------------------
# Backends
# --------------------------------------------------------------------------

FAULTS = {"qk": QK_FAULTS, "pack": PACK_FAULTS, "rope": ROPE_FAULTS,
          "gate": GATE_FAULTS, "ts": TS_FAULTS, "mlp": MLP_FAULTS}


class Emulated:
    """Plain torch in the kernels' index arithmetic and fp32 order, with an
    optional (family, fault)."""

    def __init__(self, fault=None, fused=True, rsq_ulp=0):
        self.family, self.fault = fault if fault else (None, None)
        self.fused, self.rsq_ulp = fused, rsq_ulp

    def _f(self, family):
        return self.fault if self.family == family else None

    def qk_norm_rope_(self, bufs, views, wq, wk, cs, eps):
        bufs = [b.clone() for b in bufs]
        q, k = views(bufs)
        emulate_qk_norm_rope_(q, k, wq, wk, cs, eps, self._f("qk"),
                              self.fused, self.rsq_ulp)
        return bufs

    def pack_joint_qkv(self, txt, img, wq_t, wk_t, wq_i, wk_i, cs, eps):
        return emulate_pack_joint_qkv(txt, img, wq_t, wk_t, wq_i, wk_i, cs,
                                      eps, self._f("pack"), self.fused,
                                      self.rsq_ulp)

    def rope_apply(self, x, cs):
        return emulate_rope_apply(x, cs, self._f("rope"), self.fused)[1]

    def gate_residual(self, res, gate, x):
        return emulate_gate_residual(res, gate, x, self._f("gate"))

    def gelu_tanh(self, x):
        return F8.gelu_f32(x, cancelling=True).to(x.dtype)

    def timestep_embedding(self, t, dim, max_period, time_factor):
        return emulate_timestep_embedding(t, dim, max_period, time_factor,
                                          self._f("ts"))

    def timestep_embed_mlp(self, t, w1, b1, max_period, time_factor):
        return emulate_ts_embed_mlp(t, w1, b1, max_period, time_factor,
                                    self._f("mlp"))


class OpsBackend:
    """ops.* on `device`: the reference path on the CPU, the native kernels
    on a GPU. Views are rebuilt on moved copies of their base buffers."""

    def __init__(self, device="cpu"):
        from comfyui_parallelanything_amd import ops
        self.ops, self.device = ops, device

    def to(self, t):
        return None if t is None else t.to(self.device)

    def moved_view(self, v):
        """v on the device with its strides and offset: the whole storage
        is moved and the view taken again."""
        if v.numel() == 0:
            return self.to(v)
        return torch.as_strided(self.to(_flat(v)), v.shape, v.stride(),
                                v.storage_offset())

    def qk_norm_rope_(self, bufs, views, wq, wk, cs, eps):
        dev = [self.to(b.clone()) for b in bufs]
        q, k = views(dev)
        self.ops.qk_norm_rope_(q, k, self.to(wq), self.to(wk), self.to(cs),
                               eps)
        return [b.cpu() for b in dev]

    def pack_joint_qkv(self, txt, img, wq_t, wk_t, wq_i, wk_i, cs, eps):
        td, im = self.moved_view(txt), self.moved_view(img)
        if self.device == "cpu":       # the reference path works in place
            td, im = td.clone(), im.clone()
        out = self.ops.pack_joint_qkv(
            td, im, self.to(wq_t), self.to(wk_t), self.to(wq_i),
            self.to(wk_i), self.to(cs), eps)
        return [o.cpu() for o in out]

    def rope_apply(self, x, cs):
        return self.ops.rope_apply(self.to(x), self.to(cs)).cpu()

    def gate_residual(self, res, gate, x):
        return self.ops.gate_residual(self.to(res), self.moved_view(gate),
                                      self.to(x)).cpu()

    def gelu_tanh(self, x):
        return self.ops.gelu_tanh(self.moved_view(x)).cpu()

    def timestep_embedding(self, t, dim, max_period, time_factor):
        return self.ops.timestep_embedding(self.to(t), dim, max_period,
                                           time_factor).cpu()

    def timestep_embed_mlp(self, t, w1, b1, max_period, time_factor):
        if self.device == "cpu":       # GPU-only op: the composed path
            emb = self.ops.timestep_embedding(t, w1.shape[1], max_period,
                                              time_factor)
            acc = emb @ w1.float().t()
            if b1 is not None:
                acc = acc + b1.float()
            return torch.nn.functional.silu(acc).to(BF16)
        return self.ops.timestep_embed_mlp(
            self.to(t), self.to(w1), self.to(b1), max_period,
            time_factor).cpu()


# --------------------------------------------------------------------------
# The checks: name -> function of a backend, raising AssertionError.
# --------------------------------------------------------------------------

CHECKS = {}
for _dn in DTYPES16:
    for _D in QK_DIMS:
        for _lay in QK_LAYOUTS:
            CHECKS[f"qk {_lay} quarter D={_D} {_dn}"] = _qk_check(
                _lay, "quarter", _D, _dn)
        # the other tables, one layout each (every layout meets every
        # table kind across D)
        for _i, _tab in enumerate(QK_TABLES[1:]):
            _lay = QK_LAYOUTS[(_i + _D // 2) % 3]
            CHECKS[f"qk {_lay} {_tab} D={_D} {_dn}"] = _qk_check(
                _lay, _tab, _D, _dn)
    for _D in PACK_DIMS:
        for _lay in PACK_LAYOUTS:
            for _tab in ("quarter", "model"):
                CHECKS[f"pack 3x2x3x3 {_lay} {_tab} D={_D} {_dn}"] = \
                    _pack_check(PACK_SHAPES[0], _lay, _tab, _D, _dn)
        CHECKS[f"pack 2x0x3x3 D={_D} {_dn}"] = _pack_check(
            PACK_SHAPES[1], "img_sliced", "quarter", _D, _dn)
        CHECKS[f"pack 2x3x0x3 D={_D} {_dn}"] = _pack_check(
            PACK_SHAPES[2], "txt_sliced", "quarter", _D, _dn)
    CHECKS[f"pack 4x16x16x4 all16 D=128 {_dn}"] = _pack_check(
        PACK_ALL16, "img_sliced", "quarter", 128, _dn)
    for _kind in ("vector", "strided"):
        CHECKS[f"gelu large {_kind} {_dn}"] = _gelu_check(_kind, _dn)
for _dn in DTYPES:
    for _D in ROPE_DIMS:
        for _tab in ("quarter", "model"):
            CHECKS[f"rope {_tab} D={_D} {_dn}"] = _rope_check(_tab, _D, _dn)
    for _kind in ("vec", "scalar"):
        CHECKS[f"gate {_kind} {_dn}"] = _gate_check(_kind, _dn)
        CHECKS[f"gate {_kind} {_dn} unbind"] = _gate_check(_kind, _dn, True)
CHECKS["rope large bf16"] = _rope_check("large", 256, "bf16")
CHECKS["rope large fp32"] = _rope_check("large", 256, "fp32")
CHECKS["gate large_vec bf16"] = _gate_check("large_vec", "bf16")
CHECKS["gate large_scalar bf16"] = _gate_check("large_scalar", "bf16")
CHECKS["gate large_scalar fp32"] = _gate_check("large_scalar", "fp32")
for _dim in TS_DIMS:
    for _P in TS_PERIODS:
        CHECKS[f"ts dim={_dim} P={_P:g}"] = _ts_check(_dim, _P)
CHECKS["ts large"] = ts_large
for _K in MLP_KS:
    CHECKS[f"mlp K={_K}"] = _mlp_check(_K, False)
CHECKS["mlp K=256 bias"] = _mlp_check(256, True)
CHECKS["mlp composed"] = mlp_composed

# checks whose tensors run to megabytes: the CPU file runs the emulation's
# faults on them, but ops.* on the CPU only once
LARGE = tuple(n for n in CHECKS if "large" in n)


# --------------------------------------------------------------------------
# Measurements behind SLACK and TS_A / TS_B
# --------------------------------------------------------------------------

def slack_measurements():
    """(name, worst pre-rounding error in spacings) of the fp32 emulation
    against fp64 over every 16-bit case, worst over fused / unfused
    multiply-adds and a reciprocal square root 0, +1, -1 ulp off."""
    variants = [(f, u) for f in (True, False) for u in (0, 1, -1)]
    for dn, dtype in DTYPES16.items():
        for D in QK_DIMS:
            for table in QK_TABLES:
                bufs, views, wq, wk, cs, eps, _ = qk_case("fused", table, D,
                                                          dtype)
                q, k = views(bufs)
                S = q.shape[1]
                worst = 0.0
                for x, w in ((q, wq), (k, wk)):
                    rows = x.permute(0, 2, 1, 3).reshape(-1, S, D)
                    c = cs.float()[None, :, :, 0].expand(len(rows), -1, -1)
                    s = cs.float()[None, :, :, 1].expand(len(rows), -1, -1)
                    ref = C.qk_norm_rope_f64(x, w, cs.float(), eps).permute(
                        0, 2, 1, 3).reshape(-1, D)
                    for f, u in variants:
                        v32 = rms_rope_rows(rows.reshape(-1, D), w,
                                            c.reshape(-1, D // 2),
                                            s.reshape(-1, D // 2), eps, f, u)
                        worst = max(worst, error_in_spacings(
                            v32, ref, dtype).max().item())
                yield f"qk {table} D={D} {dn}", worst
        for D in PACK_DIMS:
            txt, img, ws, cs, eps, _, _ = pack_case(
                PACK_SHAPES[0], "img_sliced", "model", D, dtype)
            rq, rk = pack_ref(txt, img, ws, cs.float(), eps)
            worst = 0.0
            for f, u in variants:
                be = _Unrounded(f, u)
                oq, ok, _ = be.pack(txt, img, ws, cs, eps)
                worst = max(worst,
                            error_in_spacings(oq, rq, dtype).max().item(),
                            error_in_spacings(ok, rk, dtype).max().item())
            yield f"pack model D={D} {dn}", worst
        for D in ROPE_DIMS:
            x, cs = rope_case("model", D, dtype)
            ref = _rope_ref(x, cs)
            worst = max(error_in_spacings(
                emulate_rope_apply(x, cs, None, f)[0], ref, dtype
            ).max().item() for f in (True, False))
            yield f"rope model D={D} {dn}", worst


class _Unrounded:
    """pack_joint_qkv's q and k before the final rounding, in fp32."""

    def __init__(self, fused, rsq_ulp):
        self.fused, self.rsq_ulp = fused, rsq_ulp

    def pack(self, txt, img, ws, cs, eps):
        T = txt.shape[1]
        outs = []
        for qkv in (0, 1):
            parts = []
            for x, w, tab in ((txt, ws[qkv], cs[:T]),
                              (img, ws[2 + qkv], cs[T:])):
                B, S, _, H, D = x.shape
                xr = x[:, :, qkv]
                c = tab.float()[None, :, None, :, 0].expand(B, S, H, -1)
                s = tab.float()[None, :, None, :, 1].expand(B, S, H, -1)
                parts.append(rms_rope_rows(
                    xr.reshape(-1, D), w, c.reshape(-1, D // 2),
                    s.reshape(-1, D // 2), eps, self.fused,
                    self.rsq_ulp).view(B, S, H, D))
            outs.append(torch.cat(parts, 1))
        return outs[0], outs[1], None


def ts_measurements():
    """(a, b) of reference.timestep_embedding (fp32 torch) against fp64 on
    the whole grid: a the worst error where |arg| <= TS_SMALL, b the worst
    of (error - a) / (|arg| 2^-24) beyond."""
    runs = [(t, dim, P, tf) for t, tf in build("ts_arguments")
            for dim in TS_DIMS for P in TS_PERIODS]
    t, dim = ts_large_case()
    runs.append((t, dim, 1e4, 1.0))
    errs, mags = [], []
    for t, dim, P, tf in runs:
        emb, mag = ts_f64(t, dim, P, tf)
        errs.append((R.timestep_embedding(t, dim, P, tf).double()
                     - emb).abs().flatten())
        mags.append(mag.flatten())
    err, mag = torch.cat(errs), torch.cat(mags)
    small = mag <= TS_SMALL
    a = err[small].max().item()
    b = ((err[~small] - a) / (mag[~small] * 2.0 ** -24)).max().item()
    return a, b


# --------------------------------------------------------------------------
# Refusals and empties: name -> function(ops, device). A refused call must
# raise RuntimeError before any launch; `AFTER` names the valid check that
# the tests run next, which would meet a pending launch error.
# --------------------------------------------------------------------------

def _z(shape, device, dtype=BF16):
    return torch.zeros(shape, dtype=dtype, device=device)


def _qk_args(device, B=2, S=3, H=2, D=8):
    cs = quarter_table(S, D // 2).to(device)
    return [_z((B, S, H, D), device), _z((B, S, H, D), device),
            _z(D, device), _z(D, device), cs]


def _pack_args(device, B=2, T=2, Si=3, H=2, D=8):
    cs = quarter_table(T + Si, D // 2).to(device)
    return ([_z((B, T, 3, H, D), device), _z((B, Si, 3, H, D), device)]
            + [_z(D, device) for _ in range(4)] + [cs])


def _swap(args, i, new):
    args = list(args)
    args[i] = new
    return args


def _refusals():
    r = {}

    def qk(name, i, make):
        def run(ops, dev):
            a = _qk_args(dev)
            ops.qk_norm_rope_(*_swap(a, i, make(a[i], dev)))
        r[f"qk {name}"] = run

    qk("k batch", 1, lambda t, d: _z((3, 3, 2, 8), d))
    qk("k head dim", 1, lambda t, d: _z((2, 3, 2, 16), d)[..., :4])
    qk("k seq", 1, lambda t, d: _z((2, 2, 2, 8), d))
    qk("cs flat", 4, lambda t, d: t.reshape(3, 8))
    qk("cs 4-d", 4, lambda t, d: t[None])
    qk("cs pairs", 4, lambda t, d: t[:, :3])
    qk("cs rows", 4, lambda t, d: t[:2])
    qk("cs last dim", 4, lambda t, d: t[..., :1])
    qk("wq short", 2, lambda t, d: _z(4, d))
    qk("wk long", 3, lambda t, d: _z(16, d))
    qk("wk 2-d", 3, lambda t, d: _z((1, 8), d))

    def pack(name, i, make):
        def run(ops, dev):
            a = _pack_args(dev)
            ops.pack_joint_qkv(*_swap(a, i, make(a[i], dev)))
        r[f"pack {name}"] = run

    pack("img batch", 1, lambda t, d: _z((3, 3, 3, 2, 8), d))
    pack("img heads", 1, lambda t, d: _z((2, 3, 3, 4, 8), d))
    pack("img head dim", 1, lambda t, d: _z((2, 3, 3, 2, 4), d))
    pack("txt qkv", 0, lambda t, d: _z((2, 2, 2, 2, 8), d))
    pack("cs rows", 6, lambda t, d: t[:4])
    pack("cs pairs", 6, lambda t, d: t[:, :2])
    pack("cs last dim", 6, lambda t, d: t[..., :1])
    pack("cs flat", 6, lambda t, d: t.reshape(5, 8))
    for i, n in ((2, "wq_t"), (3, "wk_t"), (4, "wq_i"), (5, "wk_i")):
        pack(f"{n} short", i, lambda t, d: _z(4, d))

    def gate(name, g, res=(2, 3, 8)):
        def run(ops, dev):
            ops.gate_residual(_z(res, dev), _z(g, dev), _z((2, 3, 8), dev))
        r[f"gate {name}"] = run

    gate("broadcast row", (1, 8))
    gate("wrong D", (2, 16))
    gate("wrong B", (3, 8))
    gate("residual shape", (2, 8), (2, 4, 8))
    gate("residual rows", (2, 8), (1, 3, 8))

    def rope(name, x, cs):
        def run(ops, dev):
            ops.rope_apply(_z(x, dev), _z(cs, dev, F32))
        r[f"rope {name}"] = run

    rope("odd D", (1, 2, 3, 5), (3, 2, 2))
    rope("cs pairs", (1, 2, 3, 8), (3, 3, 2))
    rope("cs rows", (1, 2, 3, 8), (2, 4, 2))
    rope("cs last dim", (1, 2, 3, 8), (3, 4, 1))
    return r


REFUSALS = _refusals()
# only with a GPU: the mismatched argument left on the CPU
DEVICE_REFUSALS = {
    "qk": (lambda ops, dev, i: ops.qk_norm_rope_(
        *_swap(_qk_args(dev), i, _qk_args("cpu")[i])), (1, 2, 3, 4)),
    "pack": (lambda ops, dev, i: ops.pack_joint_qkv(
        *_swap(_pack_args(dev), i, _pack_args("cpu")[i])),
        (1, 2, 3, 4, 5, 6)),
}


def after_refusal(name):
    return {"qk": "qk sliced quarter D=40 bf16",
            "pack": "pack 3x2x3x3 img_sliced quarter D=40 bf16",
            "gate": "gate vec bf16", "rope": "rope quarter D=6 bf16"}[
        name.split()[0]]


def _empties():
    e = {}

    def add(name, fn, shapes):
        def run(ops, dev):
            out = fn(ops, dev)
            out = out if isinstance(out, (tuple, list)) else [out]
            assert [tuple(o.shape) for o in out] == shapes, (
                name, [tuple(o.shape) for o in out])
        e[name] = run

    add("gate S=0", lambda ops, d: ops.gate_residual(
        _z((2, 0, 8), d), _z((2, 8), d), _z((2, 0, 8), d)), [(2, 0, 8)])
    add("gate B=0", lambda ops, d: ops.gate_residual(
        _z((0, 3, 8), d), _z((0, 8), d), _z((0, 3, 8), d)), [(0, 3, 8)])
    add("rope S=0", lambda ops, d: ops.rope_apply(
        _z((2, 2, 0, 8), d), _z((0, 4, 2), d, F32)), [(2, 2, 0, 8)])
    add("rope B=0", lambda ops, d: ops.rope_apply(
        _z((0, 2, 3, 8), d), _z((3, 4, 2), d, F32)), [(0, 2, 3, 8)])
    add("qk S=0", lambda ops, d: ops.qk_norm_rope_(
        *_qk_args(d, S=0)), [(2, 0, 2, 8)] * 2)
    add("qk B=0", lambda ops, d: ops.qk_norm_rope_(
        *_qk_args(d, B=0)), [(0, 3, 2, 8)] * 2)
    add("pack both empty", lambda ops, d: ops.pack_joint_qkv(
        *_pack_args(d, T=0, Si=0)), [(2, 0, 2, 8)] * 3)
    add("pack B=0", lambda ops, d: ops.pack_joint_qkv(
        *_pack_args(d, B=0)), [(0, 5, 2, 8)] * 3)
    add("gelu vector", lambda ops, d: ops.gelu_tanh(_z((2, 0, 16), d)),
        [(2, 0, 16)])
    add("gelu fp32", lambda ops, d: ops.gelu_tanh(_z((0, 5), d, F32)),
        [(0, 5)])
    add("ts B=0", lambda ops, d: ops.timestep_embedding(
        _z(0, d, F32), 8), [(0, 8)])
    add("ts dim=0", lambda ops, d: ops.timestep_embedding(
        _z(3, d, F32), 0), [(3, 0)])
    return e


EMPTIES = _empties()
