// UNet token path: affine LayerNorm with an optional fused residual add, and
// GEGLU. Kernel, then launcher. Rows here are short (320 to 1280 channels in
// SD1.5 / SDXL, 40 to 160 16-byte vectors), so the LayerNorm gives a row to
// one wave and keeps it in registers; see "UNet token ops" in
// docs/KERNELS.md.
#pragma once

// The kernels of this header are kept off the packed fp32 VALU ops
// (v_pk_add/mul/fma_f32). Those are element-wise IEEE operations and would
// give the same bits; the kernels are bound by memory and gain nothing from
// them, and with them off the instruction streams that the tests pin bit for
// bit hold scalar fp32 operations only.
#if defined(__HIP_DEVICE_COMPILE__)
#define PA_SCALAR_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PA_SCALAR_F32   // the host pass has no such feature to turn off
#endif

// ---------------------------------------------------------------------------
// Sum of v over the 64 lanes, the same bits in every lane. All VALU: DPP
// moves inside a row of 16 (quad_perm for l ^ 1 and l ^ 2, row_half_mirror
// and row_ror:8 for the other quad and the other half, which hold one value
// each by then) and the gfx950 row / half-wave swaps above that. No LDS, no
// address register, and one fixed order of additions. Every lane of the wave
// must be active.
// ---------------------------------------------------------------------------
template <int CTRL>
PA_DEV float dpp_add(float v) {
    const int i = __builtin_bit_cast(int, v);
    return v + __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, i, CTRL, 0xf, 0xf, true));
}

PA_DEV float wave_allreduce_sum(float v) {
    v = dpp_add<0xb1>(v);    // quad_perm [1,0,3,2]
    v = dpp_add<0x4e>(v);    // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);   // row_half_mirror
    v = dpp_add<0x128>(v);   // row_ror:8
    // v_permlane16_swap trades the odd rows of its first operand for the
    // even rows of its second, v_permlane32_swap the upper half for the
    // lower: given v twice, one result is the lane's own v and the other
    // its partner's
    unsigned int u = __float_as_uint(v);
    auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __uint_as_float((unsigned int)r[0]) +
        __uint_as_float((unsigned int)r[1]);
    u = __float_as_uint(v);
    r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float((unsigned int)r[0]) +
           __uint_as_float((unsigned int)r[1]);
}

// ---------------------------------------------------------------------------
// Affine LayerNorm over the last dim, one WAVE per row, four rows per
// 256-thread block: out = (x - mean) * rstd * w + b. x [rows, C] dense, CV =
// C / 8 vectors per row; lane l holds vectors l, l + 64, ... (VPL of them, so
// C <= 512 * VPL) as floats in registers from the one read to the store. No
// LDS and no barrier: a wave past the last row leaves at once.
//
// Statistics in two steps from the registers: the mean, then the sum of the
// squared deviations, which cannot round below zero and keeps its digits on
// a row that sits at an offset (E[x^2] - mean^2 loses mean^2 / var of them).
// The mean is a true division: the sum of C equal 16-bit values is exact, and
// so is its quotient by C, so a constant row comes out as exactly b. Lanes
// past CV hold zeros, are masked out of the deviations and store nothing.
//
// ADD: s = x + delta in fp32 is stored rounded to E in `sum` (the new
// residual stream) and the ROUNDED s is what gets normalised, so out is bit
// for bit the kernel's own result on `sum`.
// ---------------------------------------------------------------------------
template <typename E, int VPL, bool ADD>
__global__ __launch_bounds__(256) PA_SCALAR_F32 void layer_norm_affine_kernel(
    const E* __restrict__ x, const E* __restrict__ delta,
    const E* __restrict__ w, const E* __restrict__ b, E* __restrict__ sum,
    E* __restrict__ out, long rows, int CV, float eps) {
#pragma clang fp contract(off)   // the fused operations are written out
    using EL = Elem16<E>;
    const int lane = threadIdx.x & (WAVE - 1);
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long base = row * (long)CV;   // in vectors
    const short8* xv = reinterpret_cast<const short8*>(x) + base;
    const short8* wv = reinterpret_cast<const short8*>(w);
    const short8* bv = reinterpret_cast<const short8*>(b);
    const short8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    // every load of the row is issued here, ahead of the first reduction
    short8 xr[VPL], dr[VPL], wr[VPL], br[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = lane + i * WAVE;
        const bool live = c < CV;
        xr[i] = live ? xv[c] : zero;
        if constexpr (ADD)
            dr[i] = live ? reinterpret_cast<const short8*>(delta)[base + c]
                         : zero;
        wr[i] = live ? wv[c] : zero;
        br[i] = live ? bv[c] : zero;
    }

    float f[VPL][8];
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        if constexpr (ADD) {
            short8 s;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s[j] = (short)EL::st(EL::ld((unsigned short)xr[i][j]) +
                                     EL::ld((unsigned short)dr[i][j]));
                f[i][j] = EL::ld((unsigned short)s[j]);
            }
            const int c = lane + i * WAVE;
            if (c < CV) reinterpret_cast<short8*>(sum)[base + c] = s;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                f[i][j] = EL::ld((unsigned short)xr[i][j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += f[i][j];
    }
    const float n = (float)(CV * 8);
    const float mean = wave_allreduce_sum(acc) / n;

    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const bool live = lane + i * WAVE < CV;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f[i][j] = live ? f[i][j] - mean : 0.f;
            sq = __builtin_fmaf(f[i][j], f[i][j], sq);
        }
    }
    // once per row: the square root and the quotient, not v_rsq_f32
    const float rstd = 1.f / sqrtf(wave_allreduce_sum(sq) / n + eps);

#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = lane + i * WAVE;
        short8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = __builtin_fmaf(f[i][j] * rstd,
                                     EL::ld((unsigned short)wr[i][j]),
                                     EL::ld((unsigned short)br[i][j]));
            // the fp32 result, then the conversion: left to itself the
            // compiler fuses the two into v_fma_mixlo_f16 in some
            // instantiations and not in others, and the ADD kernel would
            // differ from the plain one on its own sum by a double rounding
            asm("" : "+v"(v));
            o[j] = (short)EL::st(v);
        }
        if (c < CV) reinterpret_cast<short8*>(out)[base + c] = o;
    }
}

static bool aligned16(const at::Tensor& t) {
    return (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) == 0;
}

static constexpr int LN_AFFINE_MAX_C = 2048;   // 4 vectors per lane

// x [rows, C] -> {out}, or with delta [rows, C]: {sum, out}, sum = x + delta
// rounded to x's dtype and out = LayerNorm(sum).
std::vector<at::Tensor> layer_norm_affine(at::Tensor x, at::Tensor weight,
                                          at::Tensor bias,
                                          std::optional<at::Tensor> delta,
                                          double eps) {
    CHECK_GPU(x);
    TORCH_CHECK(is_elem16(x.scalar_type()),
                "layer_norm_affine: bf16 or fp16, got ", x.scalar_type());
    TORCH_CHECK(x.dim() == 2, "layer_norm_affine: x [rows, C], got ",
                x.sizes());
    const long rows = x.size(0), C = x.size(1);
    TORCH_CHECK(C > 0 && C % 8 == 0 && C <= LN_AFFINE_MAX_C,
                "layer_norm_affine: C % 8 == 0 and C <= ", LN_AFFINE_MAX_C,
                ", got C = ", C);
    TORCH_CHECK(x.is_contiguous(), "layer_norm_affine: x must be contiguous "
                "(strides ", x.strides(), ")");
    TORCH_CHECK(aligned16(x), "layer_norm_affine: x must be 16-byte aligned");
    const bool add = delta.has_value();
    const at::Tensor* vecs[] = {&weight, &bias};
    for (int k = 0; k < 2; ++k) {
        const at::Tensor* t = vecs[k];
        const char* name = k == 0 ? "weight" : "bias";
        TORCH_CHECK(t->dim() == 1 && t->size(0) == C, "layer_norm_affine: ",
                    name, " must be [C] = [", C, "], got ", t->sizes());
        TORCH_CHECK(t->scalar_type() == x.scalar_type(),
                    "layer_norm_affine: ", name, " dtype (", t->scalar_type(),
                    ") must match x (", x.scalar_type(), ")");
        TORCH_CHECK(t->device() == x.device(), "layer_norm_affine: ", name,
                    " is on ", t->device(), ", x on ", x.device());
        TORCH_CHECK(t->is_contiguous() && aligned16(*t), "layer_norm_affine: ",
                    name, " must be contiguous and 16-byte aligned");
    }
    if (add) {
        TORCH_CHECK(delta->sizes() == x.sizes(), "layer_norm_affine: delta ",
                    delta->sizes(), " must have x's shape ", x.sizes());
        CHECK_SAME_DTYPE(*delta, x);
        CHECK_SAME_DEVICE(*delta, x);
        TORCH_CHECK(delta->is_contiguous() && aligned16(*delta),
                    "layer_norm_affine: delta must be contiguous and 16-byte "
                    "aligned");
    }
    TORCH_CHECK(rows <= 4L * INT_MAX, "layer_norm_affine: too many rows");
    auto out = at::empty_like(x);
    at::Tensor sum = add ? at::empty_like(x) : at::Tensor();
    if (rows > 0) {
        const int CV = (int)(C / 8);
        const dim3 grid((unsigned)((rows + 3) / 4));
        const void* dp = add ? delta->data_ptr() : nullptr;
        void* sp = add ? sum.data_ptr() : nullptr;
#define PA_LN_AFFINE(VPL, ADD)                                                \
    PA_WITH_ELEM16(x.scalar_type(), hipLaunchKernelGGL(                       \
        (layer_norm_affine_kernel<E, VPL, ADD>), grid, dim3(256), 0,          \
        cur_stream(), (const E*)x.data_ptr(), (const E*)dp,                   \
        (const E*)weight.data_ptr(), (const E*)bias.data_ptr(), (E*)sp,       \
        (E*)out.data_ptr(), rows, CV, (float)eps))
#define PA_LN_AFFINE_VPL(ADD)                                                 \
    do {                                                                      \
        if (CV <= 64) PA_LN_AFFINE(1, ADD);                                   \
        else if (CV <= 128) PA_LN_AFFINE(2, ADD);                             \
        else if (CV <= 192) PA_LN_AFFINE(3, ADD);                             \
        else PA_LN_AFFINE(4, ADD);                                            \
    } while (0)
        if (add) PA_LN_AFFINE_VPL(true);
        else PA_LN_AFFINE_VPL(false);
#undef PA_LN_AFFINE_VPL
#undef PA_LN_AFFINE
    }
    if (add) return {sum, out};
    return {out};
}

// ---------------------------------------------------------------------------
// GEGLU: out[r][c] = a * gelu(g), a = y[r][c], g = y[r][N + c]; y [rows, 2N]
// with a row stride (a column slice of a wider buffer is read in place), out
// [rows, N] dense. The exact erf GELU 0.5 * g * (1 + erf(g / sqrt 2)) in
// fp32, one rounding at the store. NV = N / 8 vectors per output row, one
// 16-byte load from each half per vector; the grid-stride loop takes two
// vectors per trip and issues their four loads before the arithmetic. The
// second vector of the last trip may not exist: it then reloads the first.
// ---------------------------------------------------------------------------
template <typename EL>
PA_DEV short8 geglu_vec8(short8 a, short8 g) {
    short8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float gf = EL::ld((unsigned short)g[j]);
        const float gelu = 0.5f * gf * (1.f + erff(gf * 0.70710678118654752f));
        o[j] = (short)EL::st(EL::ld((unsigned short)a[j]) * gelu);
    }
    return o;
}

template <typename E>
__global__ __launch_bounds__(256) PA_SCALAR_F32 void geglu_kernel(
    const E* __restrict__ y, E* __restrict__ out, long total, long NV,
    long y_rsv) {
    using EL = Elem16<E>;
    const short8* yv = reinterpret_cast<const short8*>(y);
    short8* ov = reinterpret_cast<short8*>(out);
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total;
         i += 2 * stride) {
        const bool two = i + stride < total;
        const long i1 = two ? i + stride : i;
        const long r0 = i / NV, r1 = i1 / NV;
        const long s0 = r0 * y_rsv + (i - r0 * NV);
        const long s1 = r1 * y_rsv + (i1 - r1 * NV);
        const short8 a0 = yv[s0], g0 = yv[s0 + NV];
        const short8 a1 = yv[s1], g1 = yv[s1 + NV];
        ov[i] = geglu_vec8<EL>(a0, g0);
        if (two) ov[i1] = geglu_vec8<EL>(a1, g1);
    }
}

// y [rows, 2N] (last dim contiguous, any row stride that keeps 16-byte
// alignment) -> [rows, N].
at::Tensor geglu(at::Tensor y) {
    CHECK_GPU(y);
    TORCH_CHECK(is_elem16(y.scalar_type()), "geglu: bf16 or fp16, got ",
                y.scalar_type());
    TORCH_CHECK(y.dim() == 2, "geglu: y [rows, 2N], got ", y.sizes());
    const long rows = y.size(0), W = y.size(1);
    TORCH_CHECK(W > 0 && W % 16 == 0,
                "geglu: the last dim must be 2N with N % 8 == 0, got ", W);
    TORCH_CHECK(y.stride(1) == 1,
                "geglu: the last dim must be contiguous (strides ",
                y.strides(), ")");
    TORCH_CHECK(rows <= 1 || (y.stride(0) >= 0 && y.stride(0) % 8 == 0),
                "geglu: the row stride must be a multiple of 8 elements, got ",
                y.stride(0));
    TORCH_CHECK(aligned16(y), "geglu: y must be 16-byte aligned");
    const long N = W / 2;
    auto out = at::empty({rows, N}, y.options());
    if (rows == 0) return out;
    const long NV = N / 8, total = rows * NV;
    const long y_rsv = rows > 1 ? y.stride(0) / 8 : 2 * NV;
    // two vectors per thread and trip
    const int blocks = grid_1d((total + 1) / 2);
    PA_WITH_ELEM16(y.scalar_type(), hipLaunchKernelGGL(
        geglu_kernel<E>, dim3(blocks), dim3(256), 0, cur_stream(),
        (const E*)y.data_ptr(), (E*)out.data_ptr(), total, NV, y_rsv));
    return out;
}
