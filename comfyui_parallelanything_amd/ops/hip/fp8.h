// fp8 (e4m3fn) serving mode: the shared emit helpers, the delayed-scaling
// finalize, and the three quantizing ops (quant, GELU, AdaLN LayerNorm).
#pragma once

// ---- fp8 (e4m3fn) emit: shared by layer_norm_mod_fp8_kernel,
// gelu_fp8_kernel and quant_fp8_bf16_kernel ---------------------------------
// Delayed scaling: each of the three quantizes with the scale it finds in
// scale[0] and maxes its |value| into amax_buf[0]. Nothing else happens in
// the kernel: the stream-ordered fp8_scale_finalize_kernel launched right
// after it snapshots that scale into scale_used[0], decays the amax and
// writes the next call's scale.

// Eight values f(0..7) -> clamp(f * inv_s) to the e4m3 range, cast, one
// 8-byte store at out[at]. The clamp is the NaN-propagating maximum/minimum
// pair (v_maximum3_f32 / v_minimum3_f32), so NaN in is a NaN byte out and
// +-inf saturates to +-448; fminf(fmaxf(NaN, -448), 448) is -448, the
// largest negative code. Every value that reaches the cast is then within
// +-448 or NaN, so the cast is asked for no saturation of its own: with
// __HIP_SATFINITE it clamps finite values a second time behind a test for
// inf/NaN (three instructions per element that can no longer change a
// byte). f is a callable, not an array, and the address
// is formed here, so the inlined code keeps the per-element order (value,
// amax, cast, ..., address, store) the kernels were tuned with: an array
// argument or a precomputed pointer cost 1-3 VGPRs in two of the kernels.
template <typename F>
PA_DEV void store_fp8x8(unsigned char* out, long at, float inv_s, F&& f) {
    unsigned char pack[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float q = __builtin_elementwise_minimum(
            __builtin_elementwise_maximum(f(j) * inv_s, -448.f), 448.f);
        // OCP e4m3fn cast (gfx950 format; NOT fnuz)
        pack[j] = (unsigned char)__hip_cvt_float_to_fp8(q, __HIP_NOSAT,
                                                        __HIP_E4M3);
    }
    *reinterpret_cast<unsigned long long*>(&out[at]) =
        *reinterpret_cast<unsigned long long*>(pack);
}

// Block amax -> amax_buf[0], CONDITIONAL atomicMax: thread 0 reads the
// global value plainly first and issues the atomic only when this block
// holds a new maximum, so a launch of thousands of blocks does a handful of
// real atomics. The round-2 fp8k A/B measured the scheme this replaced — a
// per-block counter chain (4096 serialized atomicAdds) for last-block
// detection — at up to ~30% of the whole kernel. Deterministic: atomicMax
// is order-independent and the finalize kernel sees the final amax.
// `scratch` holds one float per wave; every thread of the block calls this.
PA_DEV void block_amax_to_global(float local_amax, float* scratch,
                                 float* amax_buf) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        local_amax = fmaxf(local_amax, __shfl_xor(local_amax, off, 64));
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    if (lane == 0) scratch[wid] = local_amax;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = 0.f;
        for (int i = 0; i < (int)(blockDim.x / 64); ++i)
            m = fmaxf(m, scratch[i]);
        if (m > amax_buf[0])
            atomicMax(reinterpret_cast<unsigned int*>(amax_buf),
                      __float_as_uint(m));
    }
}

// Stream-ordered delayed-scaling finalize (one thread): snapshot the scale
// the preceding quantization used, decay the running amax, write the next
// call's scale. Fixed pointers -> hipGraph-capture safe. amax_buf[1] (the
// retired block counter) stays zero, preserving the public state contract.
// A running amax that is not finite (an inf activation; NaN never enters
// it) must not reach the scale, where nothing would ever bring it back:
// the scale stays as it was and the amax restarts at scale * 448.
__global__ void fp8_scale_finalize_kernel(float* scale, float* amax_buf,
                                          float* scale_used) {
    if (scale_used != scale) scale_used[0] = scale[0];
    if (!(fabsf(amax_buf[0]) < INFINITY)) {
        amax_buf[0] = scale[0] * 448.f;
        return;
    }
    const float next = amax_buf[0] * 0.999f;
    amax_buf[0] = next;
    scale[0] = fmaxf(next / 448.f, 1e-12f);
}

// Second half of every fp8-emitting op: runs after the quantizing kernel on
// the same stream (see fp8_scale_finalize_kernel).
static void fp8_scale_finalize(at::Tensor& scale, at::Tensor& amax_buf,
                               at::Tensor& scale_used) {
    hipLaunchKernelGGL(fp8_scale_finalize_kernel, dim3(1), dim3(1), 0,
                       cur_stream(), scale.data_ptr<float>(),
                       amax_buf.data_ptr<float>(),
                       scale_used.data_ptr<float>());
}

// The body of quant_fp8_bf16_kernel and gelu_fp8_kernel: out = fp8(g(x) /
// scale[0]) over total8 8-wide vectors, then the block's max |g(x)| into
// amax_buf[0]. Grid-stride with 4-deep load ILP: four independent loads in
// flight before the compute (fp8k A/B: +5% on the 16B-load/8B-store
// pattern). g maps one float to one float. The kernel passes its own first
// index and grid stride: blockDim/gridDim read inside an inlined helper miss
// the compiler's uniform-work-group fold, which cost 2 VGPRs here.
template <typename G>
PA_DEV void fp8_emit_loop(const bf16* __restrict__ x,
                          unsigned char* __restrict__ out, long total8,
                          const float* __restrict__ scale,
                          float* __restrict__ amax_buf, long first,
                          long stride, G&& g) {
    const short8* xv = reinterpret_cast<const short8*>(x);
    const float inv_s = 1.0f / scale[0];
    float local_amax = 0.f;
    for (long i = first; i < total8; i += stride * 4) {
        short8 v[4];
        long idx[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            idx[h] = i + h * stride;
            if (idx[h] < total8) v[h] = xv[idx[h]];
        }
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            if (idx[h] >= total8) break;
            store_fp8x8(out, idx[h] * 8, inv_s, [&](int j) {
                const float y = g(Elem16<bf16>::ld((unsigned short)v[h][j]));
                local_amax = fmaxf(local_amax, fabsf(y));
                return y;
            });
        }
    }
    __shared__ float scratch[8];
    block_amax_to_global(local_amax, scratch, amax_buf);
}

// One-pass bf16 -> fp8(e4m3fn) quantization with fused running amax:
// out[i] = clamp(x[i]/scale) as fp8; block-reduced |x| max atomically maxed
// into amax_buf for the NEXT call's delayed scale (no fp32 temporaries, no
// host syncs — the torch-level dynamic-quant path measured 7-12x this cost).
__global__ void quant_fp8_bf16_kernel(const bf16* __restrict__ x,
                                      unsigned char* __restrict__ out,
                                      float* __restrict__ scale,
                                      float* __restrict__ amax_buf,
                                      long total8) {
    // The value is the input's own bits, so a NaN among them can be a
    // signaling one, and fmaxf (v_max_f32 in IEEE mode) answers a signaling
    // NaN with a quiet NaN: the thread's running amax would turn NaN and
    // the next value replace it, dropping what came before. Quieted here,
    // the NaN is skipped like any other. (GELU and LayerNorm compute their
    // values, which are never signaling.)
    fp8_emit_loop(x, out, total8, scale, amax_buf,
                  (long)blockIdx.x * blockDim.x + threadIdx.x,
                  (long)gridDim.x * blockDim.x,
                  [](float f) { return __builtin_canonicalizef(f); });
}

at::Tensor quant_fp8(at::Tensor x, at::Tensor scale, at::Tensor amax_buf,
                     at::Tensor scale_used) {
    CHECK_GPU(x);
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, "quant_fp8: bf16 input");
    auto xc = x.contiguous();
    TORCH_CHECK((xc.numel() % 8) == 0, "quant_fp8: numel % 8 == 0");
    auto out = at::empty(xc.sizes(), xc.options().dtype(at::kFloat8_e4m3fn));
    const long total8 = xc.numel() / 8;
    hipLaunchKernelGGL(quant_fp8_bf16_kernel, dim3(grid_1d(total8)),
                       dim3(256), 0, cur_stream(), (const bf16*)xc.data_ptr(),
                       (unsigned char*)out.data_ptr(),
                       scale.data_ptr<float>(), amax_buf.data_ptr<float>(),
                       total8);
    // amax_buf with a second slot (the retired counter) opts into delayed
    // scaling: the finalize writes the next scale into scale[0] and
    // snapshots the scale this call quantized with into scale_used[0]
    // (pass scale_used=scale to skip the snapshot). A one-slot amax_buf
    // only accumulates the amax.
    if (amax_buf.numel() >= 2) fp8_scale_finalize(scale, amax_buf, scale_used);
    return out;
}

// tanh-GELU with the bf16 -> e4m3fn cast fused (fp8 serving mode): the
// MLP-down projection consumes the GELU output, so emitting fp8 directly
// removes its standalone quant pass. Quantizes with scale[0] and maxes
// |gelu| into amax_buf[0], like quant_fp8_bf16_kernel (see "fp8 emit").
__global__ void gelu_fp8_kernel(const bf16* __restrict__ x,
                                unsigned char* __restrict__ out, long total8,
                                float* __restrict__ scale,
                                float* __restrict__ amax_buf) {
    fp8_emit_loop(x, out, total8, scale, amax_buf,
                  (long)blockIdx.x * blockDim.x + threadIdx.x,
                  (long)gridDim.x * blockDim.x,
                  [](float f) { return gelu_tanh_f32<true>(f); });
}

at::Tensor gelu_fp8(at::Tensor x, at::Tensor scale, at::Tensor amax_buf,
                    at::Tensor scale_used) {
    CHECK_GPU(x);
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, "gelu_fp8: bf16 input");
    auto xc = x.contiguous();
    TORCH_CHECK((xc.numel() % 8) == 0, "gelu_fp8: numel % 8 == 0");
    TORCH_CHECK(amax_buf.numel() >= 2, "gelu_fp8: amax_buf needs counter");
    auto out = at::empty(xc.sizes(), xc.options().dtype(at::kFloat8_e4m3fn));
    const long total8 = xc.numel() / 8;
    hipLaunchKernelGGL(gelu_fp8_kernel, dim3(grid_1d(total8)), dim3(256), 0,
                       cur_stream(), (const bf16*)xc.data_ptr(),
                       (unsigned char*)out.data_ptr(), total8,
                       scale.data_ptr<float>(), amax_buf.data_ptr<float>());
    fp8_scale_finalize(scale, amax_buf, scale_used);
    return out;
}

// AdaLN-modulated LayerNorm with the bf16 -> fp8(e4m3fn) cast fused into
// the normalize pass (fp8 serving mode): kills the standalone quant_fp8
// pass per projection (one HBM round-trip of [B,S,D] saved per call).
// Quantizes with qscale[0] and maxes |out| into amax_buf[0] (see above).
// Block-per-row like the bf16 LN kernel (6+ TB/s): with the amax atomic
// CONDITIONAL, a 37k-block launch does only a handful of real atomics.
__global__ void layer_norm_mod_fp8_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ scale_m,
    const bf16* __restrict__ shift, unsigned char* __restrict__ out,
    int S, int D, float eps, float* __restrict__ qscale,
    float* __restrict__ amax_buf) {
    using EL = Elem16<bf16>;
    const int DV = D / 8;
    __shared__ double stats[8];
    __shared__ float scratch[8];
    const float inv_s = 1.0f / qscale[0];
    const long row = blockIdx.x;
    const long b = row / S;
    const short8* xr = reinterpret_cast<const short8*>(x + row * (long)D);
    const short8* sc = reinterpret_cast<const short8*>(scale_m + b * (long)D);
    const short8* sh = reinterpret_cast<const short8*>(shift + b * (long)D);

    float mean, rstd;
    ln_row_stats_wide<EL>(xr, D, eps, stats, mean, rstd);
    float local_amax = 0.f;
    for (int i = threadIdx.x; i < DV; i += blockDim.x) {
        short8 v = xr[i], a = sc[i], c = sh[i];
        store_fp8x8(out, row * (long)D + i * 8, inv_s, [&](int j) {
            const float f = ln_modulate<EL>(v[j], a[j], c[j], mean, rstd);
            local_amax = fmaxf(local_amax, fabsf(f));
            return f;
        });
    }
    block_amax_to_global(local_amax, scratch, amax_buf);
}

at::Tensor layer_norm_mod_fp8(at::Tensor x, at::Tensor scale, at::Tensor shift,
                              at::Tensor qscale, at::Tensor amax_buf,
                              at::Tensor scale_used, double eps) {
    CHECK_GPU(x);
    TORCH_CHECK(x.dim() == 3, "layer_norm_mod_fp8 expects [B, S, D]");
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, "bf16 input");
    auto xc = x.contiguous();
    auto sc = scale.contiguous();
    auto sh = shift.contiguous();
    const int S = (int)xc.size(1), D = (int)xc.size(2);
    TORCH_CHECK((D % 8) == 0, "layer_norm_mod_fp8: D % 8 == 0");
    CHECK_GPU(scale);
    CHECK_GPU(shift);
    CHECK_SAME_DTYPE(scale, x);
    CHECK_SAME_DTYPE(shift, x);
    TORCH_CHECK(sc.dim() == 2 && sc.size(0) == xc.size(0) && sc.size(1) == D &&
                    sc.sizes() == sh.sizes(),
                "layer_norm_mod_fp8: scale/shift [B, D]");
    TORCH_CHECK(amax_buf.numel() >= 2, "amax_buf needs the counter slot");
    auto out = at::empty(xc.sizes(), xc.options().dtype(at::kFloat8_e4m3fn));
    // block per row (bf16-LN geometry)
    const dim3 grid((unsigned)(xc.size(0) * (long)S));
    hipLaunchKernelGGL(layer_norm_mod_fp8_kernel, grid, dim3(256), 0,
                       cur_stream(), (const bf16*)xc.data_ptr(),
                       (const bf16*)sc.data_ptr(), (const bf16*)sh.data_ptr(),
                       (unsigned char*)out.data_ptr(), S, D,
                       (float)eps, qscale.data_ptr<float>(),
                       amax_buf.data_ptr<float>());
    fp8_scale_finalize(qscale, amax_buf, scale_used);
    return out;
}
