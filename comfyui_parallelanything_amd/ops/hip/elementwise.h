// Elementwise / embedding ops: gated residual, tanh-GELU, RoPE apply,
// timestep embedding and its fused MLP half. Kernel, then launcher.
#pragma once

// ---------------------------------------------------------------------------
// Gated residual: out = residual + gate[b] * x ;  x,res: [B, S, D], gate [B, D]
// with row stride g_rs (a column slice of the banked modulation GEMM is read
// in place).
// ---------------------------------------------------------------------------
template <typename T>
__global__ void gate_residual_kernel(const T* __restrict__ res,
                                     const T* __restrict__ gate,
                                     const T* __restrict__ x,
                                     T* __restrict__ out,
                                     long total, int S, int D, long g_rs) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long d = i % D;
        const long b = i / ((long)S * D);
        out[i] = (T)((float)res[i] + (float)gate[b * g_rs + d] * (float)x[i]);
    }
}

// 16-bit fast path: 8-wide gated residual; g_rsv is the gate's row stride in
// 8-element vectors
template <typename E>
__global__ void gate_residual_vec_kernel(const E* __restrict__ res,
                                         const E* __restrict__ gate,
                                         const E* __restrict__ x,
                                         E* __restrict__ out,
                                         long total8, int S, int DV,
                                         long g_rsv) {
    using EL = Elem16<E>;
    const long stride = (long)gridDim.x * blockDim.x;
    const short8* rv = reinterpret_cast<const short8*>(res);
    const short8* gv = reinterpret_cast<const short8*>(gate);
    const short8* xv = reinterpret_cast<const short8*>(x);
    short8* ov = reinterpret_cast<short8*>(out);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total8;
         i += stride) {
        const long dv = i % DV;
        const long b = i / ((long)S * DV);
        short8 r = rv[i], g = gv[b * g_rsv + dv], xx = xv[i], o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = EL::ld((unsigned short)r[j]) +
                      EL::ld((unsigned short)g[j]) *
                          EL::ld((unsigned short)xx[j]);
            o[j] = (short)EL::st(f);
        }
        ov[i] = o;
    }
}

at::Tensor gate_residual(at::Tensor res, at::Tensor gate, at::Tensor x) {
    CHECK_GPU(x);
    TORCH_CHECK(x.dim() == 3 && gate.dim() == 2,
                "gate_residual: x [B,S,D], gate [B,D]");
    // the kernels index gate[b * row_stride + d]: a broadcast [1, D] gate,
    // or one of another D, would be read past its end
    TORCH_CHECK(gate.size(0) == x.size(0) && gate.size(1) == x.size(2),
                "gate_residual: gate must be [B, D] = [", x.size(0), ", ",
                x.size(2), "], got ", gate.sizes());
    TORCH_CHECK(res.sizes() == x.sizes(), "gate_residual: residual ",
                res.sizes(), " must have x's shape ", x.sizes());
    CHECK_SAME_DEVICE(res, x);
    CHECK_SAME_DEVICE(gate, x);
    CHECK_SAME_DTYPE(res, x);
    CHECK_SAME_DTYPE(gate, x);
    if (x.numel() == 0) return at::empty(x.sizes(), x.options());
    auto rc = res.contiguous();
    auto xc = x.contiguous();
    auto out = at::empty_like(xc);
    const long total = xc.numel();
    const int S = (int)xc.size(1), D = (int)xc.size(2);
    const int blocks = grid_1d(total);
    const auto st = xc.scalar_type();
    const bool vec = is_elem16(st) && (D % 8) == 0;
    auto gc = mod_rows(gate, vec);
    const long g_rs = gc.stride(0);
    if (vec) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            gate_residual_vec_kernel<E>, dim3(blocks), dim3(256), 0,
            cur_stream(), (const E*)rc.data_ptr(), (const E*)gc.data_ptr(),
            (const E*)xc.data_ptr(), (E*)out.data_ptr(), total / 8, S, D / 8,
            g_rs / 8));
    } else {
        PA_WITH_DTYPE("gate_residual", st, hipLaunchKernelGGL(
            gate_residual_kernel<T>, dim3(blocks), dim3(256), 0,
            cur_stream(), (const T*)rc.data_ptr(), (const T*)gc.data_ptr(),
            (const T*)xc.data_ptr(), (T*)out.data_ptr(), total, S, D, g_rs));
    }
    return out;
}

// tanh-GELU of one value, g = 0.5*f*(1+tanh(c)), shared with gelu_fp8_kernel
// (fp8.h). tanh via the HARDWARE exp2 (v_exp_f32): libm tanhf measured only
// 2.7 TB/s on the bf16 pass (rocprof r02 fp8 mix). Negative-exponent form so
// exp2 never overflows (E=inf would NaN; matches tanhf to 1e-15): with
// En = exp2(-2|c|log2e) in (0,1], tanh(|c|) = (1-En)/(1+En), so
// g = f * r or f * (1-r) with r = 1/(1+En).
// 1 - r carries the rounding of r, half an ulp of 1 or more, whatever is
// left of it: 1e-5 relative at x = -3 and a third of the value at x = -5.
// A 16-bit output rounds that away (its absolute size stays below 1e-7), and
// gelu_tanh keeps the form so that its outputs stay what they were. The fp8
// emit divides by a scale that can be small, so kTail = true takes the same
// factor as En * r, which has no cancellation (same instruction count).
template <bool kTail = false>
PA_DEV float gelu_tanh_f32(float f) {
    const float c = 0.7978845608028654f * (f + 0.044715f * f * f * f);
    const float En = __builtin_amdgcn_exp2f(-2.8853900817779268f * fabsf(c));
    // v_rcp_f32 (~1 ulp) instead of the ~10-instr IEEE divide
    const float r = __builtin_amdgcn_rcpf(1.f + En);
    return f * (c >= 0.f ? r : (kTail ? En * r : 1.f - r));
}

// Vectorized tanh-GELU (16-bit short8): the MLP activation between the two
// hipBLASLt GEMMs ([B, S, 4*hidden] tensors; memory-bound).
template <typename E>
__global__ void gelu_tanh_vec_kernel(const E* __restrict__ x,
                                     E* __restrict__ out, long total8,
                                     long rows, long w8, long in_stride8) {
    using EL = Elem16<E>;
    // strided rows supported (last-dim slices of a fused projection read in
    // place — no .contiguous() copy); output is written dense.
    const long stride = (long)gridDim.x * blockDim.x;
    const short8* xv = reinterpret_cast<const short8*>(x);
    short8* ov = reinterpret_cast<short8*>(out);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total8;
         i += stride) {
        const long src = (in_stride8 == w8)
            ? i : (i / w8) * in_stride8 + (i % w8);
        short8 v = xv[src], o;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] = (short)EL::st(gelu_tanh_f32(EL::ld((unsigned short)v[j])));
        ov[i] = o;
    }
}

at::Tensor gelu_tanh(at::Tensor x) {
    CHECK_GPU(x);
    if (x.numel() == 0) return at::empty(x.sizes(), x.options());
    // accept a 2-D-decomposable strided view: last dim contiguous, all
    // leading dims collapsible to rows with ONE stride (e.g. a last-dim
    // slice of a fused projection) — avoids a .contiguous() copy.
    const int nd = x.dim();
    bool rowable = x.stride(nd - 1) == 1;
    long w = x.size(nd - 1), rows = 1, in_stride = x.stride(nd - 1) * w;
    if (rowable && nd >= 2) {
        in_stride = x.stride(nd - 2);
        rows = x.numel() / w;
        long expect = in_stride;
        for (int d = nd - 3; d >= 0; --d) {
            expect *= x.size(d + 1);
            if (x.stride(d) != expect) { rowable = false; break; }
        }
    }
    const auto st = x.scalar_type();
    // the view itself when its rows are 8-aligned, else a contiguous copy
    // read as one row
    const bool direct = is_elem16(st) && rowable && (w % 8) == 0 &&
                        (in_stride % 8) == 0;
    const at::Tensor src = direct ? x : x.contiguous();
    if (!direct) {
        rows = 1;
        w = in_stride = src.numel();
    }
    if (!is_elem16(st) || (w % 8) != 0) return at::gelu(src, "tanh");
    auto out = at::empty(x.sizes(), x.options());
    const long total8 = rows * (w / 8);
    PA_WITH_ELEM16(st, hipLaunchKernelGGL(
        gelu_tanh_vec_kernel<E>, dim3(grid_1d(total8)), dim3(256), 0,
        cur_stream(), (const E*)src.data_ptr(), (E*)out.data_ptr(),
        total8, rows, w / 8, in_stride / 8));
    return out;
}

// ---------------------------------------------------------------------------
// RoPE apply: x [B, H, S, D], cs [S, D/2, 2] fp32 -> rotate adjacent pairs.
// One thread per pair, grid-stride; bf16 pair loaded as one uint.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void rope_apply_kernel(const T* __restrict__ x,
                                  const float* __restrict__ cs,
                                  T* __restrict__ out,
                                  long total_pairs, int S, int Dh) {
    // Dh = D/2 pairs per row; cs indexed by (s, pair)
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total_pairs;
         i += stride) {
        const long pair = i % Dh;
        const long s = (i / Dh) % S;
        const float c = cs[(s * Dh + pair) * 2 + 0];
        const float sn = cs[(s * Dh + pair) * 2 + 1];
        const float x0 = (float)x[2 * i];
        const float x1 = (float)x[2 * i + 1];
        out[2 * i] = (T)(x0 * c - x1 * sn);
        out[2 * i + 1] = (T)(x0 * sn + x1 * c);
    }
}

at::Tensor rope_apply(at::Tensor x, at::Tensor cs) {
    CHECK_GPU(x);
    TORCH_CHECK(x.dim() == 4, "rope_apply expects [B, H, S, D]");
    const int S = (int)x.size(2), D = (int)x.size(3);
    // an odd D would pass cs.size(1) == D / 2 by truncation, and the pairs
    // would then straddle rows
    TORCH_CHECK(D % 2 == 0, "rope_apply: D must be even, got ", D);
    TORCH_CHECK(cs.dim() == 3 && cs.size(0) == S && cs.size(1) == D / 2 &&
                cs.size(2) == 2, "rope_apply: cs must be [S, D/2, 2] = [", S,
                ", ", D / 2, ", 2], got ", cs.sizes());
    CHECK_SAME_DEVICE(cs, x);
    if (x.numel() == 0) return at::empty(x.sizes(), x.options());
    auto xc = x.contiguous();
    auto cc = cs.to(at::kFloat).contiguous();
    auto out = at::empty_like(xc);
    const long pairs = xc.numel() / 2;
    PA_WITH_DTYPE("rope_apply", xc.scalar_type(), hipLaunchKernelGGL(
        rope_apply_kernel<T>, dim3(grid_1d(pairs)), dim3(256), 0, cur_stream(),
        (const T*)xc.data_ptr(), cc.data_ptr<float>(), (T*)out.data_ptr(),
        pairs, S, D / 2));
    return out;
}

// ---------------------------------------------------------------------------
// Timestep embedding: t [B] -> out [B, dim] fp32 (cos | sin halves).
// ---------------------------------------------------------------------------

// cos and sin of a timestep argument in radians. Not __cosf / __sinf: those
// are one multiply by 1/2pi and the hardware v_cos_f32 / v_sin_f32, which the
// ISA defines within +-256 revolutions (+-1608 rad) only, and the callers go
// beyond: t * time_factor is 4000 at FLUX's default guidance and up to 14610
// under the k-diffusion samplers. (An MI355X did wrap such arguments, with
// the error of the fp32 multiply, 3.5e-4 at 4000 rad; the manual promises
// neither.) The library functions reduce the argument over the whole fp32
// range. Both kernels are launch-bound (B * dim / 2 values), so the extra
// instructions cost nothing that can be measured.
PA_DEV void ts_cos_sin(float arg, float& c, float& s) {
    c = cosf(arg);
    s = sinf(arg);
}

__global__ void timestep_embedding_kernel(const float* __restrict__ t,
                                          float* __restrict__ out,
                                          int B, int dim, float max_period,
                                          float time_factor) {
    const int half = dim / 2;
    const long total = (long)B * half;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += stride) {
        const int b = (int)(i / half);
        const int j = (int)(i % half);
        const float freq = __expf(-__logf(max_period) * (float)j / (float)half);
        const float arg = t[b] * time_factor * freq;
        float c, sn;
        ts_cos_sin(arg, c, sn);
        out[(long)b * dim + j] = c;
        out[(long)b * dim + half + j] = sn;
        if ((dim & 1) && j == 0) out[(long)b * dim + dim - 1] = 0.f;
    }
}

at::Tensor timestep_embedding(at::Tensor t, long dim, double max_period,
                              double time_factor) {
    CHECK_GPU(t);
    TORCH_CHECK(t.dim() == 1 && dim >= 0,
                "timestep_embedding: t [B] and dim >= 0, got t ", t.sizes(),
                ", dim ", dim);
    auto tc = t.to(at::kFloat).contiguous();
    const int B = (int)tc.size(0);
    // dim 0 and 1 have no cos/sin pair: the kernel would write nothing (the
    // odd column hangs on j == 0); dim 1 is that zero column alone
    if (B == 0 || dim < 2) return at::zeros({B, dim}, tc.options());
    auto out = at::empty({B, dim}, tc.options());
    const int blocks = (int)std::min<long>((B * (dim / 2) + 255) / 256, 1024);
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(std::max(blocks, 1)),
                       dim3(256), 0, cur_stream(), tc.data_ptr<float>(),
                       out.data_ptr<float>(), B, (int)dim, (float)max_period,
                       (float)time_factor);
    return out;
}

// ---------------------------------------------------------------------------
// Fused timestep-embedding MLP input half: out = silu(sinusoid(t) @ W1^T + b1)
// (SURVEY §2b "sinusoidal + 2xLinear+SiLU fused"; the out_layer Linear is a
// GEMM-shaped op and stays on hipBLASLt). One 256-thread block covers 256
// hidden outputs of one batch element; the K-dim sinusoid is computed once
// into LDS per block. B is tiny (<=32) so this stage is launch-bound —
// collapsing embed+linear+silu into one kernel removes two launches and the
// [B,K] fp32 + bf16-cast intermediates (and keeps the sinusoid fp32 into
// the accumulate, slightly MORE accurate than the cast-then-GEMM path).
// ---------------------------------------------------------------------------
__global__ void ts_embed_mlp_kernel(const float* __restrict__ t,
                                    const bf16* __restrict__ w1,  // [H, K]
                                    const bf16* __restrict__ b1,  // [H]|null
                                    bf16* __restrict__ out,       // [B, H]
                                    int H, int K,
                                    float max_period, float time_factor) {
    extern __shared__ float emb[];  // [K]
    const int hblocks = (H + 255) / 256;
    const int b = blockIdx.x / hblocks;
    const int hblk = blockIdx.x % hblocks;
    const int half = K / 2;
    const float tv = t[b] * time_factor;
    for (int j = (int)threadIdx.x; j < half; j += (int)blockDim.x) {
        const float freq = __expf(-__logf(max_period) * (float)j / (float)half);
        const float arg = tv * freq;
        float c, sn;
        ts_cos_sin(arg, c, sn);
        emb[j] = c;
        emb[half + j] = sn;
    }
    __syncthreads();
    const int o = hblk * 256 + (int)threadIdx.x;
    if (o >= H) return;
    float acc = b1 ? bf2f(b1[o]) : 0.f;
    const short8* wrow = reinterpret_cast<const short8*>(w1 + (long)o * K);
    for (int k8 = 0; k8 < K / 8; ++k8) {
        const short8 w = wrow[k8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            acc += emb[k8 * 8 + j] *
                   bf2f(__ushort_as_bfloat16((unsigned short)w[j]));
    }
    acc = acc / (1.f + __expf(-acc));  // SiLU
    out[(long)b * H + o] = f2bf(acc);
}

at::Tensor timestep_embed_mlp(at::Tensor t, at::Tensor w1,
                              c10::optional<at::Tensor> b1,
                              double max_period, double time_factor) {
    CHECK_GPU(t);
    TORCH_CHECK(w1.scalar_type() == at::kBFloat16,
                "timestep_embed_mlp: bf16 weight");
    TORCH_CHECK(w1.dim() == 2, "timestep_embed_mlp: w1 [H, K], got ",
                w1.sizes());
    CHECK_SAME_DEVICE(w1, t);
    auto tc = t.to(at::kFloat).contiguous();
    auto w1c = w1.contiguous();
    const int H = (int)w1c.size(0), K = (int)w1c.size(1);
    TORCH_CHECK(K % 8 == 0 && K <= 4096,
                "timestep_embed_mlp: K % 8 == 0 and K <= 4096");
    const int B = (int)tc.numel();
    auto out = at::empty({B, H}, w1c.options());
    const bf16* bias = nullptr;
    at::Tensor b1c;
    if (b1.has_value()) {
        CHECK_SAME_DEVICE(*b1, t);
        b1c = b1->contiguous();
        TORCH_CHECK(b1c.scalar_type() == at::kBFloat16 &&
                    (int)b1c.numel() == H, "timestep_embed_mlp: bias [H] bf16");
        bias = (const bf16*)b1c.data_ptr();
    }
    if (B == 0 || H == 0) return out;
    const int hblocks = (H + 255) / 256;
    hipLaunchKernelGGL(ts_embed_mlp_kernel, dim3(B * hblocks), dim3(256),
                       K * sizeof(float), cur_stream(), tc.data_ptr<float>(),
                       (const bf16*)w1c.data_ptr(), bias,
                       (bf16*)out.data_ptr(), H, K, (float)max_period,
                       (float)time_factor);
    return out;
}
