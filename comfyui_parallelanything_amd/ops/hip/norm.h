// RMSNorm, AdaLN-modulated LayerNorm and GroupNorm+SiLU: kernels, each
// followed by its launcher.
#pragma once

// ---------------------------------------------------------------------------
// RMSNorm: one 256-thread block per row, vectorized bf16x8 loads (G13).
// rows = prod(leading dims), D = last dim.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void rms_norm_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                T* __restrict__ out, int D, float eps) {
    const long row = blockIdx.x;
    const T* xr = x + row * (long)D;
    T* yr = out + row * (long)D;
    __shared__ float scratch[8];

    float acc = 0.f;
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        float v = (float)xr[i];
        acc += v * v;
    }
    float ssq = block_reduce_sum<256>(acc, scratch);
    const float rrms = rsqrtf(ssq / (float)D + eps);
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        float v = (float)xr[i] * rrms;
        if (w != nullptr) v *= (float)w[i];
        yr[i] = (T)v;
    }
}

// 16-bit fast path (E = bf16 | _Float16): 8-wide vector loads/stores.
template <typename E>
__global__ void rms_norm_vec_kernel(const E* __restrict__ x,
                                    const E* __restrict__ w,
                                    E* __restrict__ out, int D, float eps) {
    using EL = Elem16<E>;
    const long row = blockIdx.x;
    const short8* xr = reinterpret_cast<const short8*>(x + row * (long)D);
    short8* yr = reinterpret_cast<short8*>(out + row * (long)D);
    const short8* wv = reinterpret_cast<const short8*>(w);
    const int DV = D / 8;
    __shared__ float scratch[8];

    float acc = 0.f;
    for (int i = threadIdx.x; i < DV; i += blockDim.x) {
        short8 v = xr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = EL::ld((unsigned short)v[j]);
            acc += f * f;
        }
    }
    float ssq = block_reduce_sum<256>(acc, scratch);
    const float rrms = rsqrtf(ssq / (float)D + eps);
    for (int i = threadIdx.x; i < DV; i += blockDim.x) {
        short8 v = xr[i];
        short8 o;
        if (w != nullptr) {
            short8 wv8 = wv[i];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float f = EL::ld((unsigned short)v[j]) * rrms *
                          EL::ld((unsigned short)wv8[j]);
                o[j] = (short)EL::st(f);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float f = EL::ld((unsigned short)v[j]) * rrms;
                o[j] = (short)EL::st(f);
            }
        }
        yr[i] = o;
    }
}

// Small-D fast path (qk-norm: D = head_dim 64..256): one WAVE per row, four
// rows per 256-thread block; pair loads (uint = 2 elements) when D % 128 == 0.
template <typename E>
__global__ void rms_norm_row_kernel(const E* __restrict__ x,
                                    const E* __restrict__ w,
                                    E* __restrict__ out,
                                    long rows, int D, float eps) {
    using EL = Elem16<E>;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const unsigned int* xr =
        reinterpret_cast<const unsigned int*>(x + row * (long)D);
    unsigned int* yr = reinterpret_cast<unsigned int*>(out + row * (long)D);
    const unsigned int* wr = reinterpret_cast<const unsigned int*>(w);
    const int P = D / 2;  // pairs per row
    float acc = 0.f;
    unsigned int vals[4];  // up to D=512
    const int n = P / 64 + ((lane < (P % 64)) ? 1 : 0);
    for (int i = 0; i < n; ++i) {
        unsigned int u = xr[lane + i * 64];
        vals[i] = u;
        float a = EL::ld((unsigned short)(u & 0xffff));
        float b = EL::ld((unsigned short)(u >> 16));
        acc += a * a + b * b;
    }
    acc = wave_reduce_sum(acc);
    const float rrms = rsqrtf(acc / (float)D + eps);
    for (int i = 0; i < n; ++i) {
        unsigned int u = vals[i];
        float a = EL::ld((unsigned short)(u & 0xffff)) * rrms;
        float b = EL::ld((unsigned short)(u >> 16)) * rrms;
        if (w != nullptr) {
            unsigned int uw = wr[lane + i * 64];
            a *= EL::ld((unsigned short)(uw & 0xffff));
            b *= EL::ld((unsigned short)(uw >> 16));
        }
        yr[lane + i * 64] =
            (unsigned int)EL::st(a) | ((unsigned int)EL::st(b) << 16);
    }
}

at::Tensor rms_norm(at::Tensor x, std::optional<at::Tensor> w, double eps) {
    CHECK_GPU(x);
    auto xc = x.contiguous();
    auto out = at::empty_like(xc);
    const long rows = xc.numel() / xc.size(-1);
    const int D = (int)xc.size(-1);
    at::Tensor wc;
    if (w.has_value()) {
        wc = w->contiguous();
        TORCH_CHECK(wc.scalar_type() == xc.scalar_type(), "weight dtype mismatch");
    }
    const auto st = xc.scalar_type();
    const void* wptr = w.has_value() ? wc.data_ptr() : nullptr;
    if (is_elem16(st) && (D % 128) == 0 && D <= 512) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            rms_norm_row_kernel<E>, dim3((unsigned)((rows + 3) / 4)),
            dim3(256), 0, cur_stream(), (const E*)xc.data_ptr(),
            (const E*)wptr, (E*)out.data_ptr(), rows, D, (float)eps));
    } else if (is_elem16(st) && (D % 8) == 0) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            rms_norm_vec_kernel<E>, dim3((unsigned)rows), dim3(256), 0,
            cur_stream(), (const E*)xc.data_ptr(), (const E*)wptr,
            (E*)out.data_ptr(), D, (float)eps));
    } else {
        PA_WITH_DTYPE("rms_norm", st, hipLaunchKernelGGL(
            rms_norm_kernel<T>, dim3((unsigned)rows), dim3(256), 0,
            cur_stream(), (const T*)xc.data_ptr(), (const T*)wptr,
            (T*)out.data_ptr(), D, (float)eps));
    }
    return out;
}

// ---------------------------------------------------------------------------
// AdaLN-modulated LayerNorm: out = LN(x) * (1 + scale[b]) + shift[b].
// x: [B, S, D]; scale/shift: [B, D] with row strides sc_rs / sh_rs in
// elements (column slices of one banked modulation GEMM are read in place).
// One block per (b, s) row.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void layer_norm_mod_kernel(const T* __restrict__ x,
                                      const T* __restrict__ scale,
                                      const T* __restrict__ shift,
                                      T* __restrict__ out,
                                      int S, int D, long sc_rs, long sh_rs,
                                      float eps) {
    const long row = blockIdx.x;          // b * S + s
    const long b = row / S;
    const T* xr = x + row * (long)D;
    const T* sc = scale + b * sc_rs;
    const T* sh = shift + b * sh_rs;
    T* yr = out + row * (long)D;
    __shared__ float scratch[8];

    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        float v = (float)xr[i];
        s1 += v;
        s2 += v * v;
    }
    // two reductions share the scratch sequentially
    float mean = block_reduce_sum<256>(s1, scratch) / (float)D;
    // single-pass E[x^2] - mean^2 can round below zero on a (near-)constant
    // row, and rsqrtf of that is NaN: clamp (exact whenever var >= 0)
    float var = block_reduce_sum<256>(s2, scratch) / (float)D - mean * mean;
    float corr = 0.f;
    if constexpr (sizeof(T) == 4) {
        // fp32 rows are held to 1e-5. The difference above loses mean^2 /
        // var of fp32's digits (4e-4 off at mean 40, variance 1), and the
        // mean itself is only good to its own rounding (2e-6 at 40). A pass
        // over the deviations d = x - mean gives both back: var = E[d^2] -
        // E[d]^2, and E[d] is what the mean missed.
        float sd = 0.f, sq = 0.f;
        for (int i = threadIdx.x; i < D; i += blockDim.x) {
            float d = (float)xr[i] - mean;
            sd += d;
            sq += d * d;
        }
        corr = block_reduce_sum<256>(sd, scratch) / (float)D;
        var = block_reduce_sum<256>(sq, scratch) / (float)D - corr * corr;
    }
    const float rstd = rsqrtf(fmaxf(var, 0.f) + eps);
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        float v = (float)xr[i] - mean;
        if constexpr (sizeof(T) == 4) v -= corr;
        v *= rstd;
        v = v * (1.f + (float)sc[i]) + (float)sh[i];
        yr[i] = (T)v;
    }
}

// The 16-bit vector form of the two passes, shared with
// layer_norm_mod_fp8_kernel (fp8.h). Row statistics: every thread of the
// 256-thread block gets the row's mean and rstd; the two reductions share
// `scratch` (8 floats) sequentially.
template <typename EL>
PA_DEV f32x2 ln_row_sums(const short8* xr, int D) {
    // (sum, sum of squares) as one explicit pair: the compiler pairs the
    // two scalar sums into v_pk_add_f32 when the loop is written in the
    // kernel, but not when it is inlined from here
    f32x2 s = {0.f, 0.f};
    for (int i = threadIdx.x; i < D / 8; i += blockDim.x) {
        short8 v = xr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = EL::ld((unsigned short)v[j]);
            s += f32x2{f, f * f};
        }
    }
    return s;
}

template <typename EL>
PA_DEV void ln_row_stats(const short8* xr, int D, float eps, float* scratch,
                         float& mean, float& rstd) {
    const f32x2 s = ln_row_sums<EL>(xr, D);
    mean = block_reduce_sum<256>(s[0], scratch) / (float)D;
    // clamped for layer_norm_mod_kernel's reason
    float var = block_reduce_sum<256>(s[1], scratch) / (float)D - mean * mean;
    rstd = rsqrtf(fmaxf(var, 0.f) + eps);
}

// The same statistics with the two sums reduced across the block, and the
// variance taken, in fp64 (layer_norm_mod_fp8_kernel). var = E[x^2] - mean^2
// loses mean^2 / var of the digits it is computed in: on a row of mean 40
// and variance 1 the fp32 form leaves rstd 5e-5 to 1.5e-4 off, which a
// 16-bit output rounds away but the fp8 emit carries into its running amax
// and from there into the next scale. The per-thread sums stay fp32, the
// loop above: a thread adds at most D / 2048 vectors, and where the
// cancellation is large the row's values share a binade or two, so the
// squares of bf16 values (16 bits) add exactly in 24. `scratch` holds two
// doubles per wave; one exchange instead of two.
template <typename EL>
PA_DEV void ln_row_stats_wide(const short8* xr, int D, float eps,
                              double* scratch, float& mean, float& rstd) {
    const f32x2 s = ln_row_sums<EL>(xr, D);
    double s1 = s[0], s2 = s[1];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off, 64);
        s2 += __shfl_xor(s2, off, 64);
    }
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    if (lane == 0) {
        scratch[2 * wid] = s1;
        scratch[2 * wid + 1] = s2;
    }
    __syncthreads();
    s1 = (scratch[0] + scratch[2]) + (scratch[4] + scratch[6]);
    s2 = (scratch[1] + scratch[3]) + (scratch[5] + scratch[7]);
    const double inv_d = 1.0 / (double)D;
    const double m = s1 * inv_d;
    mean = (float)m;
    rstd = rsqrtf(fmaxf((float)(s2 * inv_d - m * m), 0.f) + eps);
}

// Normalize and modulate one element: (x - mean) * rstd * (1 + scale) + shift.
template <typename EL>
PA_DEV float ln_modulate(short x, short scale, short shift, float mean,
                         float rstd) {
    float f = (EL::ld((unsigned short)x) - mean) * rstd;
    return f * (1.f + EL::ld((unsigned short)scale)) +
           EL::ld((unsigned short)shift);
}

// 16-bit fast path: short8 vector loads both passes (mean/var re-read hits L2)
template <typename E>
__global__ void layer_norm_mod_vec_kernel(const E* __restrict__ x,
                                          const E* __restrict__ scale,
                                          const E* __restrict__ shift,
                                          E* __restrict__ out,
                                          int S, int D, long sc_rs,
                                          long sh_rs, float eps) {
    using EL = Elem16<E>;
    const long row = blockIdx.x;
    const long b = row / S;
    const short8* xr = reinterpret_cast<const short8*>(x + row * (long)D);
    const short8* sc = reinterpret_cast<const short8*>(scale + b * sc_rs);
    const short8* sh = reinterpret_cast<const short8*>(shift + b * sh_rs);
    short8* yr = reinterpret_cast<short8*>(out + row * (long)D);
    const int DV = D / 8;
    __shared__ float scratch[8];

    float mean, rstd;
    ln_row_stats<EL>(xr, D, eps, scratch, mean, rstd);
    for (int i = threadIdx.x; i < DV; i += blockDim.x) {
        short8 v = xr[i], a = sc[i], c = sh[i], o;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] = (short)EL::st(ln_modulate<EL>(v[j], a[j], c[j], mean, rstd));
        yr[i] = o;
    }
}

at::Tensor layer_norm_mod(at::Tensor x, at::Tensor scale, at::Tensor shift,
                          double eps) {
    CHECK_GPU(x);
    TORCH_CHECK(x.dim() == 3, "layer_norm_mod expects [B, S, D]");
    auto xc = x.contiguous();
    TORCH_CHECK(scale.sizes() == shift.sizes() && scale.dim() == 2,
                "scale/shift [B, D]");
    auto out = at::empty_like(xc);
    const int B = (int)xc.size(0), S = (int)xc.size(1), D = (int)xc.size(2);
    // the kernels index scale[b * row_stride + d]
    TORCH_CHECK(scale.size(0) == B && scale.size(1) == D,
                "layer_norm_mod: scale/shift must be [B, D] = [", B, ", ", D,
                "], got ", scale.sizes());
    dim3 grid((unsigned)((long)B * S));
    const auto st = xc.scalar_type();
    CHECK_SAME_DTYPE(scale, x);
    CHECK_SAME_DTYPE(shift, x);
    CHECK_SAME_DEVICE(scale, x);
    CHECK_SAME_DEVICE(shift, x);
    if (xc.numel() == 0) return out;
    const bool vec = is_elem16(st) && (D % 8) == 0;
    auto sc = mod_rows(scale, vec);
    auto sh = mod_rows(shift, vec);
    const long sc_rs = sc.stride(0), sh_rs = sh.stride(0);
    if (vec) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            layer_norm_mod_vec_kernel<E>, grid, dim3(256), 0, cur_stream(),
            (const E*)xc.data_ptr(), (const E*)sc.data_ptr(),
            (const E*)sh.data_ptr(), (E*)out.data_ptr(), S, D, sc_rs, sh_rs,
            (float)eps));
    } else {
        PA_WITH_DTYPE("layer_norm_mod", st, hipLaunchKernelGGL(
            layer_norm_mod_kernel<T>, grid, dim3(256), 0, cur_stream(),
            (const T*)xc.data_ptr(), (const T*)sc.data_ptr(),
            (const T*)sh.data_ptr(), (T*)out.data_ptr(), S, D, sc_rs, sh_rs,
            (float)eps));
    }
    return out;
}

// ---------------------------------------------------------------------------
// GroupNorm + SiLU: x [B, C, H, W]; one block per (b, group).
// ---------------------------------------------------------------------------
template <typename T>
__global__ void group_norm_silu_kernel(const T* __restrict__ x,
                                       const float* __restrict__ w,
                                       const float* __restrict__ bias,
                                       T* __restrict__ out,
                                       int C, long HW, int G, float eps) {
    const int b = blockIdx.x / G;
    const int g = blockIdx.x % G;
    const int cpg = C / G;
    const long base = ((long)b * C + (long)g * cpg) * HW;
    const long n = (long)cpg * HW;
    __shared__ float scratch[8];

    float s1 = 0.f, s2 = 0.f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        float v = (float)x[base + i];
        s1 += v;
        s2 += v * v;
    }
    float mean = block_reduce_sum<256>(s1, scratch) / (float)n;
    // clamped, and for fp32 corrected by a pass over the deviations, for
    // layer_norm_mod_kernel's reasons
    float var = block_reduce_sum<256>(s2, scratch) / (float)n - mean * mean;
    float corr = 0.f;
    if constexpr (sizeof(T) == 4) {
        float sd = 0.f, sq = 0.f;
        for (long i = threadIdx.x; i < n; i += blockDim.x) {
            float d = (float)x[base + i] - mean;
            sd += d;
            sq += d * d;
        }
        corr = block_reduce_sum<256>(sd, scratch) / (float)n;
        var = block_reduce_sum<256>(sq, scratch) / (float)n - corr * corr;
    }
    const float rstd = rsqrtf(fmaxf(var, 0.f) + eps);
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const int c = g * cpg + (int)(i / HW);
        float v = (float)x[base + i] - mean;
        if constexpr (sizeof(T) == 4) v -= corr;
        v *= rstd;
        if (w != nullptr) v = v * w[c] + bias[c];
        out[base + i] = (T)(v / (1.f + __expf(-v)));  // SiLU
    }
}

at::Tensor group_norm_silu(at::Tensor x, long groups,
                           std::optional<at::Tensor> w,
                           std::optional<at::Tensor> b, double eps) {
    CHECK_GPU(x);
    TORCH_CHECK(x.dim() == 4, "group_norm_silu expects [B, C, H, W]");
    auto xc = x.contiguous();
    auto out = at::empty_like(xc);
    const int B = (int)xc.size(0), C = (int)xc.size(1);
    const long HW = (long)xc.size(2) * xc.size(3);
    TORCH_CHECK(C % groups == 0, "C % groups != 0");
    at::Tensor wf, bf;
    const float *wp = nullptr, *bp = nullptr;
    if (w.has_value()) {
        wf = w->to(at::kFloat).contiguous();
        bf = b.has_value() ? b->to(at::kFloat).contiguous()
                           : at::zeros({C}, wf.options());
        wp = wf.data_ptr<float>();
        bp = bf.data_ptr<float>();
    }
    dim3 grid((unsigned)(B * groups));
    PA_WITH_DTYPE("group_norm_silu", xc.scalar_type(), hipLaunchKernelGGL(
        group_norm_silu_kernel<T>, grid, dim3(256), 0, cur_stream(),
        (const T*)xc.data_ptr(), wp, bp, (T*)out.data_ptr(), C, HW,
        (int)groups, (float)eps));
    return out;
}
