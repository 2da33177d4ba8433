// MI355X (gfx950, CDNA4) native kernels for comfyui_parallelanything_amd.
//
// Hand-written HIP: fused attention (MFMA 16x16x32 bf16, LDS-tiled),
// AdaLN-modulated LayerNorm, RMSNorm, GroupNorm+SiLU, RoPE apply, gated
// residual, timestep embedding. No CUDA-compat shims, no hipify: this file
// targets gfx950 only (wave64, 4xSIMD-32 CUs, 160 KiB LDS, per-XCD L2).
//
// These replace the per-step model math the reference node left to stock
// PyTorch inside ComfyUI's model implementations: the
// reference repo has no native code, so every kernel here is new work
// driven by the behavioral contract of the ops/reference.py functions,
// which are the fp32 ground truth in tests/test_gpu_kernels.py.
//
// Build: ops/build.py (hipcc --offload-arch=gfx950, in-tree .so).

#include <torch/extension.h>
#include <vector>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_fp8.h>

#define PA_DEV __device__ __forceinline__

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(8))) short short8;   // 8 x bf16 (4 VGPR)
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short short4v;  // 4 x bf16
typedef __attribute__((ext_vector_type(2))) float f32x2;

static constexpr int WAVE = 64;

PA_DEV float bf2f(bf16 v) { return __bfloat162float(v); }
PA_DEV bf16 f2bf(float v) { return __float2bfloat16(v); }

// ---------------------------------------------------------------------------
// 16-bit element trait: bf16 and fp16 share every vector width, LDS layout
// and lane shuffle (short8 / uint stay the storage types); only the
// conversions and the MFMA opcode differ.
//   ld / st : raw 16-bit lane <-> float (st rounds to nearest even)
//   pack2   : two floats -> one packed 32-bit word (lo in bits 0..15)
//   mfma32  : v_mfma_f32_32x32x16_{bf16,f16}
// The build defines __HIP_NO_HALF_OPERATORS__/__HIP_NO_HALF_CONVERSIONS__, so
// fp16 is the native _Float16, never __half.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) _Float16 half8;
typedef __attribute__((ext_vector_type(2))) _Float16 half2v;

template <typename E> struct Elem16;

template <> struct Elem16<bf16> {
    static PA_DEV float ld(unsigned short u) {
        return bf2f(__ushort_as_bfloat16(u));
    }
    static PA_DEV unsigned short st(float f) {
        return __bfloat16_as_ushort(f2bf(f));
    }
    static PA_DEV unsigned int pack2(float lo, float hi) {
        unsigned int r;
        asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
        return r;
    }
    static PA_DEV f32x16 mfma32(short8 a, short8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

template <> struct Elem16<_Float16> {
    static PA_DEV float ld(unsigned short u) {
        return (float)__builtin_bit_cast(_Float16, u);
    }
    static PA_DEV unsigned short st(float f) {
        return __builtin_bit_cast(unsigned short, (_Float16)f);
    }
    static PA_DEV unsigned int pack2(float lo, float hi) {
        // one v_cvt_pk_f16_f32 (RNE) — not the round-toward-zero cvt_pkrtz
        return __builtin_bit_cast(
            unsigned int, __builtin_convertvector(f32x2{lo, hi}, half2v));
    }
    static PA_DEV f32x16 mfma32(short8 a, short8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(
            __builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c,
            0, 0, 0);
    }
};

// ---------------------------------------------------------------------------
// Wave/block reductions (wave64; lane groups via __shfl_xor over 64 lanes).
// ---------------------------------------------------------------------------
PA_DEV float wave_reduce_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int BLOCK>
PA_DEV float block_reduce_sum(float v, float* scratch) {
    constexpr int NW = BLOCK / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    v = wave_reduce_sum(v);
    __syncthreads();  // protect scratch against the previous reduction's reads
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) total += scratch[i];  // LDS broadcast reads
    return total;
}

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

// ---------------------------------------------------------------------------
// AdaLN-modulated LayerNorm: out = LN(x) * (1 + scale[b]) + shift[b].
// x: [B, S, D]; scale/shift: [B, D]. One block per (b, s) row.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void layer_norm_mod_kernel(const T* __restrict__ x,
                                      const T* __restrict__ scale,
                                      const T* __restrict__ shift,
                                      T* __restrict__ out,
                                      int S, int D, float eps) {
    const long row = blockIdx.x;          // b * S + s
    const long b = row / S;
    const T* xr = x + row * (long)D;
    const T* sc = scale + b * (long)D;
    const T* sh = shift + b * (long)D;
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
    float var = block_reduce_sum<256>(s2, scratch) / (float)D - mean * mean;
    const float rstd = rsqrtf(var + eps);
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        float v = ((float)xr[i] - mean) * rstd;
        v = v * (1.f + (float)sc[i]) + (float)sh[i];
        yr[i] = (T)v;
    }
}

// ---------------------------------------------------------------------------
// Gated residual: out = residual + gate[b] * x ;  x,res: [B, S, D], gate [B, D]
// ---------------------------------------------------------------------------
template <typename T>
__global__ void gate_residual_kernel(const T* __restrict__ res,
                                     const T* __restrict__ gate,
                                     const T* __restrict__ x,
                                     T* __restrict__ out,
                                     long total, int S, int D) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long d = i % D;
        const long b = i / ((long)S * D);
        out[i] = (T)((float)res[i] + (float)gate[b * D + d] * (float)x[i]);
    }
}


// 16-bit fast path: short8 vector loads both passes (mean/var re-read hits L2)
template <typename E>
__global__ void layer_norm_mod_vec_kernel(const E* __restrict__ x,
                                          const E* __restrict__ scale,
                                          const E* __restrict__ shift,
                                          E* __restrict__ out,
                                          int S, int D, float eps) {
    using EL = Elem16<E>;
    const long row = blockIdx.x;
    const long b = row / S;
    const short8* xr = reinterpret_cast<const short8*>(x + row * (long)D);
    const short8* sc = reinterpret_cast<const short8*>(scale + b * (long)D);
    const short8* sh = reinterpret_cast<const short8*>(shift + b * (long)D);
    short8* yr = reinterpret_cast<short8*>(out + row * (long)D);
    const int DV = D / 8;
    __shared__ float scratch[8];

    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < DV; i += blockDim.x) {
        short8 v = xr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = EL::ld((unsigned short)v[j]);
            s1 += f;
            s2 += f * f;
        }
    }
    float mean = block_reduce_sum<256>(s1, scratch) / (float)D;
    float var = block_reduce_sum<256>(s2, scratch) / (float)D - mean * mean;
    const float rstd = rsqrtf(var + eps);
    for (int i = threadIdx.x; i < DV; i += blockDim.x) {
        short8 v = xr[i], a = sc[i], c = sh[i], o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = (EL::ld((unsigned short)v[j]) - mean) * rstd;
            f = f * (1.f + EL::ld((unsigned short)a[j])) +
                EL::ld((unsigned short)c[j]);
            o[j] = (short)EL::st(f);
        }
        yr[i] = o;
    }
}


// ---- fp8 (e4m3fn) emit: shared by layer_norm_mod_fp8_kernel,
// gelu_fp8_kernel and quant_fp8_bf16_kernel ---------------------------------
// Delayed scaling: each of the three quantizes with the scale it finds in
// scale[0] and maxes its |value| into amax_buf[0]. Nothing else happens in
// the kernel: the stream-ordered fp8_scale_finalize_kernel launched right
// after it snapshots that scale into scale_used[0], decays the amax and
// writes the next call's scale.

// Eight values f(0..7) -> clamp(f * inv_s) to the e4m3 range, cast, one
// 8-byte store at out[at]. f is a callable, not an array, and the address
// is formed here, so the inlined code keeps the per-element order (value,
// amax, cast, ..., address, store) the kernels were tuned with: an array
// argument or a precomputed pointer cost 1-3 VGPRs in two of the kernels.
template <typename F>
PA_DEV void store_fp8x8(unsigned char* out, long at, float inv_s, F&& f) {
    unsigned char pack[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float q = fminf(fmaxf(f(j) * inv_s, -448.f), 448.f);
        // OCP e4m3fn cast (gfx950 format; NOT fnuz)
        pack[j] = (unsigned char)__hip_cvt_float_to_fp8(q, __HIP_SATFINITE,
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

// AdaLN-modulated LayerNorm with the bf16 -> fp8(e4m3fn) cast fused into
// the normalize pass (fp8 serving mode): kills the standalone quant_fp8
// pass per projection (one HBM round-trip of [B,S,D] saved per call).
// Quantizes with qscale[0] and maxes |out| into amax_buf[0] (see above).
__global__ void layer_norm_mod_fp8_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ scale_m,
    const bf16* __restrict__ shift, unsigned char* __restrict__ out,
    long n_rows, int S, int D, float eps, float* __restrict__ qscale,
    float* __restrict__ amax_buf) {
    const int DV = D / 8;
    __shared__ float scratch[8];
    const float inv_s = 1.0f / qscale[0];

    // Block-per-row like the bf16 LN kernel (6+ TB/s): with the amax atomic
    // CONDITIONAL, a 37k-block launch does only a handful of real atomics —
    // the earlier grid-stride detour (latency-bound at 2.3 TB/s) is no
    // longer needed.
    float local_amax = 0.f;
    const long row = blockIdx.x;
    if (row < n_rows) {
        const long b = row / S;
        const short8* xr = reinterpret_cast<const short8*>(x + row * (long)D);
        const short8* sc =
            reinterpret_cast<const short8*>(scale_m + b * (long)D);
        const short8* sh =
            reinterpret_cast<const short8*>(shift + b * (long)D);

        float s1 = 0.f, s2 = 0.f;
        for (int i = threadIdx.x; i < DV; i += blockDim.x) {
            short8 v = xr[i];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float f = bf2f(__ushort_as_bfloat16((unsigned short)v[j]));
                s1 += f;
                s2 += f * f;
            }
        }
        float mean = block_reduce_sum<256>(s1, scratch) / (float)D;
        float var = block_reduce_sum<256>(s2, scratch) / (float)D - mean * mean;
        const float rstd = rsqrtf(var + eps);
        for (int i = threadIdx.x; i < DV; i += blockDim.x) {
            short8 v = xr[i], a = sc[i], c = sh[i];
            store_fp8x8(out, row * (long)D + i * 8, inv_s, [&](int j) {
                float f = (bf2f(__ushort_as_bfloat16((unsigned short)v[j])) - mean) * rstd;
                f = f * (1.f + bf2f(__ushort_as_bfloat16((unsigned short)a[j]))) +
                    bf2f(__ushort_as_bfloat16((unsigned short)c[j]));
                local_amax = fmaxf(local_amax, fabsf(f));
                return f;
            });
        }
    }
    // scratch reuse: stragglers may still read the reduce broadcast
    __syncthreads();
    block_amax_to_global(local_amax, scratch, amax_buf);
}

// 16-bit fast path: 8-wide gated residual
template <typename E>
__global__ void gate_residual_vec_kernel(const E* __restrict__ res,
                                         const E* __restrict__ gate,
                                         const E* __restrict__ x,
                                         E* __restrict__ out,
                                         long total8, int S, int DV) {
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
        short8 r = rv[i], g = gv[b * DV + dv], xx = xv[i], o;
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


// tanh-GELU with the bf16 -> e4m3fn cast fused (fp8 serving mode): the
// MLP-down projection consumes the GELU output, so emitting fp8 directly
// removes its standalone quant pass. Quantizes with scale[0] and maxes
// |gelu| into amax_buf[0], like quant_fp8_bf16_kernel (see "fp8 emit").
__global__ void gelu_fp8_kernel(const bf16* __restrict__ x,
                                unsigned char* __restrict__ out, long total8,
                                float* __restrict__ scale,
                                float* __restrict__ amax_buf) {
    const long stride = (long)gridDim.x * blockDim.x;
    const short8* xv = reinterpret_cast<const short8*>(x);
    const float inv_s = 1.0f / scale[0];
    float local_amax = 0.f;
    // 4-deep ILP: four independent loads in flight before the compute
    // (fp8k A/B: +5% on this pattern)
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total8;
         i += stride * 4) {
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
                const float f =
                    bf2f(__ushort_as_bfloat16((unsigned short)v[h][j]));
                const float c =
                    0.7978845608028654f * (f + 0.044715f * f * f * f);
                // tanh via the HARDWARE exp2 (v_exp_f32), negative-exponent
                // form so exp2 never overflows (matches tanhf to 1e-15):
                // g = 0.5*f*(1+tanh(c)); En = exp2(-2|c|log2e) in (0,1]
                const float En =
                    __builtin_amdgcn_exp2f(-2.8853900817779268f * fabsf(c));
                // v_rcp_f32 (~1 ulp) instead of the ~10-instr IEEE divide
                const float r = __builtin_amdgcn_rcpf(1.f + En);
                const float g = f * (c >= 0.f ? r : 1.f - r);
                local_amax = fmaxf(local_amax, fabsf(g));
                return g;
            });
        }
    }
    __shared__ float scratch[8];
    block_amax_to_global(local_amax, scratch, amax_buf);
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
        for (int j = 0; j < 8; ++j) {
            const float f = EL::ld((unsigned short)v[j]);
            const float c = 0.7978845608028654f * (f + 0.044715f * f * f * f);
            // tanh via the HARDWARE exp2 (v_exp_f32): libm tanhf measured
            // only 2.7 TB/s on this pass (rocprof r02 fp8 mix). Negative-
            // exponent form so exp2 never overflows (E=inf would NaN):
            // g = 0.5*f*(1+tanh(c)); with En = exp2(-2|c|log2e) in (0,1],
            // tanh(|c|) = (1-En)/(1+En) -> g = f * r or f * (1-r).
            const float En =
                __builtin_amdgcn_exp2f(-2.8853900817779268f * fabsf(c));
            // v_rcp_f32 (~1 ulp) instead of the ~10-instr IEEE divide
                const float r = __builtin_amdgcn_rcpf(1.f + En);
            const float g = f * (c >= 0.f ? r : 1.f - r);
            o[j] = (short)EL::st(g);
        }
        ov[i] = o;
    }
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
    float var = block_reduce_sum<256>(s2, scratch) / (float)n - mean * mean;
    const float rstd = rsqrtf(var + eps);
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const int c = g * cpg + (int)(i / HW);
        float v = ((float)x[base + i] - mean) * rstd;
        if (w != nullptr) v = v * w[c] + bias[c];
        out[base + i] = (T)(v / (1.f + __expf(-v)));  // SiLU
    }
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

// ---------------------------------------------------------------------------
// Timestep embedding: t [B] -> out [B, dim] fp32 (cos | sin halves).
// ---------------------------------------------------------------------------
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
        out[(long)b * dim + j] = __cosf(arg);
        out[(long)b * dim + half + j] = __sinf(arg);
        if ((dim & 1) && j == 0) out[(long)b * dim + dim - 1] = 0.f;
    }
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
        emb[j] = __cosf(arg);
        emb[half + j] = __sinf(arg);
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


// ---------------------------------------------------------------------------
// Fused qk-norm + RoPE (in-place): per (b, s, h) row of q and k,
// RMSNorm over D with per-head-dim weight, then rotary by cs[s].
// One wave handles one (b, s, h) row of BOTH q and k — single pass over the
// qkv projection output (strided [B, S, H, D] views), replacing four
// separate bandwidth passes (rms q, rms k, rope q, rope k).
// ---------------------------------------------------------------------------
template <typename E>
__global__ void qk_norm_rope_kernel(E* __restrict__ q, E* __restrict__ k,
                                    const E* __restrict__ wq,
                                    const E* __restrict__ wk,
                                    const float* __restrict__ cs,
                                    int S, int H, int D,
                                    long q_bs, long q_hs, long q_ss,
                                    long k_bs, long k_hs, long k_ss,
                                    long n_rows, float eps) {
    using EL = Elem16<E>;
    // RPW rows of q AND k per wave with all loads issued before any
    // reduction: 8 independent loads in flight per lane instead of 2
    // (the single-row version measured latency-bound at ~650 GB/s).
    constexpr int RPW = 4;
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int pairs = D / 2;
    // D < 128 leaves lanes >= pairs with no data, but they MUST stay alive
    // through the 64-lane __shfl_xor reductions below (an early return here
    // would feed undefined registers into the cross-lane sum): inactive
    // lanes load from a clamped address, contribute 0, and skip the store.
    const bool act = lane < pairs;
    const int ln = act ? lane : 0;

    unsigned int uq[RPW], uk[RPW];
    unsigned int* qp[RPW];
    unsigned int* kp[RPW];
    float cvec[RPW], svec[RPW];
    const unsigned int uwq = reinterpret_cast<const unsigned int*>(wq)[ln];
    const unsigned int uwk = reinterpret_cast<const unsigned int*>(wk)[ln];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const long row = wave * RPW + i;
        const long rr = row < n_rows ? row : n_rows - 1;
        const long b = rr / ((long)S * H);
        const long sh = rr % ((long)S * H);
        const int sj = (int)(sh / H);
        const int h = (int)(sh % H);
        qp[i] = reinterpret_cast<unsigned int*>(
            q + b * q_bs + (long)sj * q_ss + (long)h * q_hs);
        kp[i] = reinterpret_cast<unsigned int*>(
            k + b * k_bs + (long)sj * k_ss + (long)h * k_hs);
        uq[i] = qp[i][ln];
        uk[i] = kp[i][ln];
        cvec[i] = cs[((long)sj * pairs + ln) * 2 + 0];
        svec[i] = cs[((long)sj * pairs + ln) * 2 + 1];
    }
    const float wq0 = EL::ld((unsigned short)(uwq & 0xffff));
    const float wq1 = EL::ld((unsigned short)(uwq >> 16));
    const float wk0 = EL::ld((unsigned short)(uwk & 0xffff));
    const float wk1 = EL::ld((unsigned short)(uwk >> 16));
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        if (wave * RPW + i >= n_rows) break;
        {
            float a0 = EL::ld((unsigned short)(uq[i] & 0xffff));
            float a1 = EL::ld((unsigned short)(uq[i] >> 16));
            float ss_ = act ? a0 * a0 + a1 * a1 : 0.f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                ss_ += __shfl_xor(ss_, off, 64);
            const float rr = rsqrtf(ss_ / (float)D + eps);
            a0 = a0 * rr * wq0;
            a1 = a1 * rr * wq1;
            const float o0 = a0 * cvec[i] - a1 * svec[i];
            const float o1 = a0 * svec[i] + a1 * cvec[i];
            if (act)
                qp[i][lane] = (unsigned int)EL::st(o0) |
                              ((unsigned int)EL::st(o1) << 16);
        }
        {
            float a0 = EL::ld((unsigned short)(uk[i] & 0xffff));
            float a1 = EL::ld((unsigned short)(uk[i] >> 16));
            float ss_ = act ? a0 * a0 + a1 * a1 : 0.f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                ss_ += __shfl_xor(ss_, off, 64);
            const float rr = rsqrtf(ss_ / (float)D + eps);
            a0 = a0 * rr * wk0;
            a1 = a1 * rr * wk1;
            const float o0 = a0 * cvec[i] - a1 * svec[i];
            const float o1 = a0 * svec[i] + a1 * cvec[i];
            if (act)
                kp[i][lane] = (unsigned int)EL::st(o0) |
                              ((unsigned int)EL::st(o1) << 16);
        }
    }
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
    const long stride = (long)gridDim.x * blockDim.x;
    const short8* xv = reinterpret_cast<const short8*>(x);
    const float inv_s = 1.0f / scale[0];
    float local_amax = 0.f;
    // 4-deep load ILP (fp8k A/B: +5% on the 16B-load/8B-store pattern)
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total8;
         i += stride * 4) {
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
                const float f =
                    bf2f(__ushort_as_bfloat16((unsigned short)v[h][j]));
                local_amax = fmaxf(local_amax, fabsf(f));
                return f;
            });
        }
    }
    __shared__ float scratch[8];
    block_amax_to_global(local_amax, scratch, amax_buf);
}


// Stream-ordered delayed-scaling finalize (one thread): snapshot the scale
// the preceding quantization used, decay the running amax, write the next
// call's scale. Fixed pointers -> hipGraph-capture safe. amax_buf[1] (the
// retired block counter) stays zero, preserving the public state contract.
__global__ void fp8_scale_finalize_kernel(float* scale, float* amax_buf,
                                          float* scale_used) {
    if (scale_used != scale) scale_used[0] = scale[0];
    const float next = amax_buf[0] * 0.999f;
    amax_buf[0] = next;
    scale[0] = fmaxf(next / 448.f, 1e-12f);
}

// ---------------------------------------------------------------------------
// Fused attention forward (flash-style, non-causal), bf16, D in {64, 128}.
//
// v2 geometry: 512-thread workgroups (8 waves). Each wave owns QBLK=32
// query rows (two 16-row M-tiles); a workgroup covers 256 rows of one
// (batch, head). K/V stream through LDS in KVBLK=64-key tiles,
// double-buffered through REGISTERS (T14 async-stage split: issue tile
// t+1's global loads right after the barrier, write them to LDS at the top
// of iteration t+1 — HBM latency hides under tile t's 64 MFMAs per wave).
//
// MFMA v_mfma_f32_16x16x32_bf16 for QK^T and P*V; online softmax in the
// exp2 domain (hardware v_exp_f32 is exp2; saves a VALU mul per element);
// per-row running (m, l) reduced across the C-fragment's 16-lane groups.
//
// LDS layouts (conflict-free by row padding, guide §6 G4; strides chosen so
// 16 consecutive rows hit 16 distinct bank groups):
//   K tile : [KVBLK][D + 8]        row stride 272 B (D=128): i*68 dw % 64 distinct
//   V tile : [D][KVBLK + 8]        TRANSPOSED at stage time (PV B-fragment
//                                   wants 8 consecutive keys per lane)
//   P tile : per-wave [32][KVBLK + 8]
// ---------------------------------------------------------------------------
using bf16x8 = short8;
typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;

PA_DEV f32x4 mfma16x16x32(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

#define PA_LOG2E 1.4426950408889634f

template <int D>
__global__ __launch_bounds__(512, 2) void attn_fwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, bf16* __restrict__ out,
    int S, int Sk, float scale, int H,
    long q_bs, long q_hs, int q_ss,
    long k_bs, long k_hs, int k_ss,
    long v_bs, long v_hs, int v_ss,
    long o_bs, long o_hs, int o_ss) {
    constexpr int KVBLK = 64;
    constexpr int QBLK = 32;          // per wave
    constexpr int WAVES = 8;
    constexpr int THREADS = WAVES * 64;
    constexpr int KPAD = D + 8;       // K row stride (elements)
    constexpr int VPAD = KVBLK + 8;   // V^T row stride
    constexpr int PPAD = KVBLK + 8;
    constexpr int KK = D / 32;        // MFMA K-steps per QK 16-col tile
    constexpr int ND = D / 16;        // PV output col tiles
    constexpr int NKC = KVBLK / 16;   // QK col tiles per KV tile (4)
    constexpr int NPS = KVBLK / 32;   // PV K-steps per KV tile (2)
    // per-thread staging share: KVBLK*D elements over THREADS threads
    constexpr int KVECS = (KVBLK * D) / (8 * THREADS);   // b128 pieces each

    __shared__ bf16 k_lds[KVBLK * KPAD];
    __shared__ bf16 v_lds[D * VPAD];
    __shared__ bf16 p_lds[WAVES * QBLK * PPAD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l16 = lane & 15;        // fragment row / col within 16
    const int lg = lane >> 4;         // 16-lane group id (0..3)

    const long bh = blockIdx.y;
    const long b = bh / H;
    const int h = (int)(bh % H);
    const int q0 = blockIdx.x * (WAVES * QBLK) + wid * QBLK;

    const bf16* qp = q + b * q_bs + (long)h * q_hs;
    const bf16* kp = k + b * k_bs + (long)h * k_hs;
    const bf16* vp = v + b * v_bs + (long)h * v_hs;
    bf16* op = out + b * o_bs + (long)h * o_hs;

    // ---- Q fragments (A-layout): lane holds Q[m*16 + l16][kk*32 + lg*8 + j]
    bf16x8 qfrag[2][KK];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int row = q0 + m * 16 + l16;
        const int rr = row < S ? row : (S > 0 ? S - 1 : 0);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
            qfrag[m][kk] = *reinterpret_cast<const bf16x8*>(
                qp + (long)rr * q_ss + kk * 32 + lg * 8);
    }

    f32x4 o_acc[2][ND];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < ND; ++n) o_acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[2][4], l_run[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) { m_run[m][r] = -1e30f; l_run[m][r] = 0.f; }

    bf16* my_p = p_lds + wid * QBLK * PPAD;
    const float scale2 = scale * PA_LOG2E;   // softmax in exp2 domain

    // ---- register prefetch state: each thread stages KVECS b128 pieces of
    //      K and of V. Piece i covers row = (tid + i*THREADS) / (D/8),
    //      col8 = (tid + i*THREADS) % (D/8).
    bf16x8 kreg[KVECS], vreg[KVECS];

    auto issue_tile_loads = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < KVECS; ++i) {
            const int idx = tid + i * THREADS;
            const int row = idx / (D / 8);
            const int col = (idx % (D / 8)) * 8;
            const int src = kv0 + row;
            if (src < Sk) {
                kreg[i] = *reinterpret_cast<const bf16x8*>(kp + (long)src * k_ss + col);
                vreg[i] = *reinterpret_cast<const bf16x8*>(vp + (long)src * v_ss + col);
            } else {
                kreg[i] = bf16x8{0,0,0,0,0,0,0,0};
                vreg[i] = bf16x8{0,0,0,0,0,0,0,0};
            }
        }
    };

    auto write_tile_lds = [&]() {
#pragma unroll
        for (int i = 0; i < KVECS; ++i) {
            const int idx = tid + i * THREADS;
            const int row = idx / (D / 8);
            const int col = (idx % (D / 8)) * 8;
            *reinterpret_cast<bf16x8*>(&k_lds[row * KPAD + col]) = kreg[i];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int dim = col + j;
                // granule-XOR swizzle: keys permuted in 8-wide granules by
                // (dim>>3)&7; read side applies the same XOR (G4 / T2).
                const int key_swz =
                    (((row >> 3) ^ ((dim >> 3) & 7)) << 3) | (row & 7);
                v_lds[dim * VPAD + key_swz] =
                    __ushort_as_bfloat16((unsigned short)vreg[i][j]);
            }
        }
    };

    issue_tile_loads(0);

    const int n_tiles = (Sk + KVBLK - 1) / KVBLK;
    for (int t = 0; t < n_tiles; ++t) {
        const int kv0 = t * KVBLK;
        __syncthreads();           // previous tile's LDS reads complete
        write_tile_lds();
        __syncthreads();           // tile ready
        if (t + 1 < n_tiles) issue_tile_loads(kv0 + KVBLK);  // overlap w/ MFMAs

        // ---- QK^T: 2 M-tiles x NKC col tiles x KK K-steps ----------------
        f32x4 s_acc[2][NKC];
#pragma unroll
        for (int n = 0; n < NKC; ++n) {
            const int key = n * 16 + l16;
            bf16x8 bfrag[KK];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                bfrag[kk] = *reinterpret_cast<const bf16x8*>(
                    &k_lds[key * KPAD + kk * 32 + lg * 8]);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                s_acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KK; ++kk)
                    s_acc[m][n] = mfma16x16x32(qfrag[m][kk], bfrag[kk], s_acc[m][n]);
            }
            __builtin_amdgcn_s_setprio(0);
        }

        // ---- online softmax (exp2 domain) --------------------------------
        bool key_ok[NKC];
#pragma unroll
        for (int n = 0; n < NKC; ++n) key_ok[n] = (kv0 + n * 16 + l16) < Sk;

        bool all_skip = true;
        float mx_mr[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float mx = -1e30f;
#pragma unroll
                for (int n = 0; n < NKC; ++n) {
                    const float sv = key_ok[n] ? s_acc[m][n][r] * scale2 : -1e30f;
                    s_acc[m][n][r] = sv;
                    mx = fmaxf(mx, sv);
                }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1)
                    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
                mx_mr[m][r] = mx;
                all_skip = all_skip && (mx <= m_run[m][r]);
            }
        }
        // exact defer: when NO row's max grew (common on late tiles),
        // alpha == exp2(0) == 1 exactly -> skip the O-accumulator rescale
        const bool skip = __all(all_skip);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float mnew = skip ? m_run[m][r]
                                        : fmaxf(m_run[m][r], mx_mr[m][r]);
                float ps = 0.f;
#pragma unroll
                for (int n = 0; n < NKC; ++n) {
                    const float pv_ = exp2f(s_acc[m][n][r] - mnew);
                    ps += pv_;
                    s_acc[m][n][r] = pv_;
                }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1)
                    ps += __shfl_xor(ps, off, 64);
                if (!skip) {
                    const float alpha = exp2f(m_run[m][r] - mnew);
                    m_run[m][r] = mnew;
                    l_run[m][r] = l_run[m][r] * alpha + ps;
#pragma unroll
                    for (int n = 0; n < ND; ++n) o_acc[m][n][r] *= alpha;
                } else {
                    l_run[m][r] += ps;
                }
            }
        }

        // ---- P -> LDS (bf16), then PV ------------------------------------
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NKC; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    my_p[(m * 16 + lg * 4 + r) * PPAD + n * 16 + l16] =
                        f2bf(s_acc[m][n][r]);
        // wave-local LDS write->read: drain lgkm (hipcc also tracks these).
        __builtin_amdgcn_s_waitcnt(/*lgkmcnt(0) vmcnt(max)*/ 0xc07f);
#pragma unroll
        for (int ks = 0; ks < NPS; ++ks) {
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                bf16x8 pa = *reinterpret_cast<const bf16x8*>(
                    &my_p[(m * 16 + l16) * PPAD + ks * 32 + lg * 8]);
#pragma unroll
                for (int n = 0; n < ND; ++n) {
                    const int dim = n * 16 + l16;
                    const int gsw = ((ks * 4 + lg) ^ ((dim >> 3) & 7)) << 3;
                    bf16x8 vb = *reinterpret_cast<const bf16x8*>(
                        &v_lds[dim * VPAD + gsw]);
                    o_acc[m][n] = mfma16x16x32(pa, vb, o_acc[m][n]);
                }
            }
        }
    }

    // ---- epilogue: O / l, store -------------------------------------------
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = q0 + m * 16 + lg * 4 + r;
            if (row >= S) continue;
            const float inv_l =
                (l_run[m][r] > 0.f) ? 1.f / l_run[m][r] : 0.f;
#pragma unroll
            for (int n = 0; n < ND; ++n)
                op[(long)row * o_ss + n * 16 + l16] =
                    f2bf(o_acc[m][n][r] * inv_l);
        }
}

// ===========================================================================
// Host-side launchers / torch bindings
// ===========================================================================

#define CHECK_GPU(t) TORCH_CHECK((t).is_cuda(), #t " must be on a HIP device")
#define CHECK_LASTDIM(t) TORCH_CHECK((t).stride(-1) == 1, #t " last dim must be contiguous")

// The kernels take raw pointers: every tensor whose pointer is cast to the
// element type of `ref` must carry ref's dtype, or an fp16 buffer would be
// read by a bf16 instantiation (and vice versa).
#define CHECK_SAME_DTYPE(t, ref)                                              \
    TORCH_CHECK((t).scalar_type() == (ref).scalar_type(),                     \
                #t " dtype (", (t).scalar_type(), ") must match " #ref " (",  \
                (ref).scalar_type(), ")")

static hipStream_t cur_stream() {
    return c10::hip::getCurrentHIPStream().stream();
}

static bool is_elem16(at::ScalarType t) {
    return t == at::kBFloat16 || t == at::kHalf;
}

// Runs the statement(s) with `E` bound to the kernels' element type for a
// 16-bit scalar type (caller has checked is_elem16).
#define PA_WITH_ELEM16(ST, ...)                                               \
    do {                                                                      \
        if ((ST) == at::kBFloat16) { using E = bf16; __VA_ARGS__; }           \
        else { using E = _Float16; __VA_ARGS__; }                             \
    } while (0)

// Second half of every fp8-emitting op: runs after the quantizing kernel on
// the same stream (see fp8_scale_finalize_kernel).
static void fp8_scale_finalize(at::Tensor& scale, at::Tensor& amax_buf,
                               at::Tensor& scale_used) {
    hipLaunchKernelGGL(fp8_scale_finalize_kernel, dim3(1), dim3(1), 0,
                       cur_stream(), scale.data_ptr<float>(),
                       amax_buf.data_ptr<float>(),
                       scale_used.data_ptr<float>());
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
    } else if (st == at::kFloat) {
        hipLaunchKernelGGL(rms_norm_kernel<float>, dim3((unsigned)rows), dim3(256), 0,
                           cur_stream(), xc.data_ptr<float>(),
                           w.has_value() ? wc.data_ptr<float>() : nullptr,
                           out.data_ptr<float>(), D, (float)eps);
    } else if (is_elem16(st)) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            rms_norm_kernel<E>, dim3((unsigned)rows), dim3(256), 0,
            cur_stream(), (const E*)xc.data_ptr(), (const E*)wptr,
            (E*)out.data_ptr(), D, (float)eps));
    } else {
        TORCH_CHECK(false, "rms_norm: unsupported dtype ", st,
                    " (bf16, fp16 or fp32)");
    }
    return out;
}

at::Tensor layer_norm_mod(at::Tensor x, at::Tensor scale, at::Tensor shift,
                          double eps) {
    CHECK_GPU(x);
    TORCH_CHECK(x.dim() == 3, "layer_norm_mod expects [B, S, D]");
    auto xc = x.contiguous();
    auto sc = scale.contiguous();
    auto sh = shift.contiguous();
    TORCH_CHECK(sc.sizes() == sh.sizes() && sc.dim() == 2, "scale/shift [B, D]");
    auto out = at::empty_like(xc);
    const int B = (int)xc.size(0), S = (int)xc.size(1), D = (int)xc.size(2);
    dim3 grid((unsigned)((long)B * S));
    const auto st = xc.scalar_type();
    CHECK_SAME_DTYPE(scale, x);
    CHECK_SAME_DTYPE(shift, x);
    if (is_elem16(st) && (D % 8) == 0) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            layer_norm_mod_vec_kernel<E>, grid, dim3(256), 0, cur_stream(),
            (const E*)xc.data_ptr(), (const E*)sc.data_ptr(),
            (const E*)sh.data_ptr(), (E*)out.data_ptr(), S, D, (float)eps));
    } else if (is_elem16(st)) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            layer_norm_mod_kernel<E>, grid, dim3(256), 0, cur_stream(),
            (const E*)xc.data_ptr(), (const E*)sc.data_ptr(),
            (const E*)sh.data_ptr(), (E*)out.data_ptr(), S, D, (float)eps));
    } else if (st == at::kFloat) {
        hipLaunchKernelGGL(layer_norm_mod_kernel<float>, grid, dim3(256), 0,
                           cur_stream(), xc.data_ptr<float>(),
                           sc.data_ptr<float>(), sh.data_ptr<float>(),
                           out.data_ptr<float>(), S, D, (float)eps);
    } else {
        TORCH_CHECK(false, "layer_norm_mod: unsupported dtype ", st,
                    " (bf16, fp16 or fp32)");
    }
    return out;
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
    TORCH_CHECK(amax_buf.numel() >= 2, "amax_buf needs the counter slot");
    auto out = at::empty(xc.sizes(), xc.options().dtype(at::kFloat8_e4m3fn));
    const long n_rows = xc.size(0) * (long)S;
    const dim3 grid((unsigned)n_rows);  // block per row (bf16-LN geometry)
    hipLaunchKernelGGL(layer_norm_mod_fp8_kernel, grid, dim3(256), 0,
                       cur_stream(), (const bf16*)xc.data_ptr(),
                       (const bf16*)sc.data_ptr(), (const bf16*)sh.data_ptr(),
                       (unsigned char*)out.data_ptr(), n_rows, S, D,
                       (float)eps, qscale.data_ptr<float>(),
                       amax_buf.data_ptr<float>());
    fp8_scale_finalize(qscale, amax_buf, scale_used);
    return out;
}

at::Tensor gate_residual(at::Tensor res, at::Tensor gate, at::Tensor x) {
    CHECK_GPU(x);
    TORCH_CHECK(x.dim() == 3 && gate.dim() == 2, "x [B,S,D], gate [B,D]");
    auto rc = res.contiguous();
    auto gc = gate.contiguous();
    auto xc = x.contiguous();
    auto out = at::empty_like(xc);
    const long total = xc.numel();
    const int S = (int)xc.size(1), D = (int)xc.size(2);
    const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
    const auto st = xc.scalar_type();
    CHECK_SAME_DTYPE(res, x);
    CHECK_SAME_DTYPE(gate, x);
    if (is_elem16(st) && (D % 8) == 0) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            gate_residual_vec_kernel<E>, dim3(blocks), dim3(256), 0,
            cur_stream(), (const E*)rc.data_ptr(), (const E*)gc.data_ptr(),
            (const E*)xc.data_ptr(), (E*)out.data_ptr(), total / 8, S, D / 8));
    } else if (is_elem16(st)) {
        PA_WITH_ELEM16(st, hipLaunchKernelGGL(
            gate_residual_kernel<E>, dim3(blocks), dim3(256), 0,
            cur_stream(), (const E*)rc.data_ptr(), (const E*)gc.data_ptr(),
            (const E*)xc.data_ptr(), (E*)out.data_ptr(), total, S, D));
    } else if (st == at::kFloat) {
        hipLaunchKernelGGL(gate_residual_kernel<float>, dim3(blocks), dim3(256), 0,
                           cur_stream(), rc.data_ptr<float>(), gc.data_ptr<float>(),
                           xc.data_ptr<float>(), out.data_ptr<float>(), total, S, D);
    } else {
        TORCH_CHECK(false, "gate_residual: unsupported dtype ", st,
                    " (bf16, fp16 or fp32)");
    }
    return out;
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
    if (is_elem16(xc.scalar_type())) {
        PA_WITH_ELEM16(xc.scalar_type(), hipLaunchKernelGGL(
            group_norm_silu_kernel<E>, grid, dim3(256), 0, cur_stream(),
            (const E*)xc.data_ptr(), wp, bp, (E*)out.data_ptr(), C, HW,
            (int)groups, (float)eps));
    } else if (xc.scalar_type() == at::kFloat) {
        hipLaunchKernelGGL(group_norm_silu_kernel<float>, grid, dim3(256), 0,
                           cur_stream(), xc.data_ptr<float>(), wp, bp,
                           out.data_ptr<float>(), C, HW, (int)groups, (float)eps);
    } else {
        TORCH_CHECK(false, "group_norm_silu: unsupported dtype ",
                    xc.scalar_type(), " (bf16, fp16 or fp32)");
    }
    return out;
}

at::Tensor rope_apply(at::Tensor x, at::Tensor cs) {
    CHECK_GPU(x);
    TORCH_CHECK(x.dim() == 4, "rope_apply expects [B, H, S, D]");
    TORCH_CHECK(cs.dim() == 3, "cs expects [S, D/2, 2]");
    auto xc = x.contiguous();
    auto cc = cs.to(at::kFloat).contiguous();
    auto out = at::empty_like(xc);
    const int S = (int)xc.size(2), D = (int)xc.size(3);
    TORCH_CHECK((int)cc.size(0) == S && (int)cc.size(1) == D / 2, "cs shape");
    const long pairs = xc.numel() / 2;
    const int blocks = (int)std::min<long>((pairs + 255) / 256, 4096);
    if (is_elem16(xc.scalar_type())) {
        PA_WITH_ELEM16(xc.scalar_type(), hipLaunchKernelGGL(
            rope_apply_kernel<E>, dim3(blocks), dim3(256), 0, cur_stream(),
            (const E*)xc.data_ptr(), cc.data_ptr<float>(),
            (E*)out.data_ptr(), pairs, S, D / 2));
    } else if (xc.scalar_type() == at::kFloat) {
        hipLaunchKernelGGL(rope_apply_kernel<float>, dim3(blocks), dim3(256), 0,
                           cur_stream(), xc.data_ptr<float>(),
                           cc.data_ptr<float>(), out.data_ptr<float>(),
                           pairs, S, D / 2);
    } else {
        TORCH_CHECK(false, "rope_apply: unsupported dtype ",
                    xc.scalar_type(), " (bf16, fp16 or fp32)");
    }
    return out;
}

at::Tensor timestep_embedding(at::Tensor t, long dim, double max_period,
                              double time_factor) {
    CHECK_GPU(t);
    auto tc = t.to(at::kFloat).contiguous();
    const int B = (int)tc.size(0);
    auto out = at::empty({B, dim}, tc.options());
    const int blocks = (int)std::min<long>((B * (dim / 2) + 255) / 256, 1024);
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(std::max(blocks, 1)),
                       dim3(256), 0, cur_stream(), tc.data_ptr<float>(),
                       out.data_ptr<float>(), B, (int)dim, (float)max_period,
                       (float)time_factor);
    return out;
}


at::Tensor timestep_embed_mlp(at::Tensor t, at::Tensor w1,
                              c10::optional<at::Tensor> b1,
                              double max_period, double time_factor) {
    CHECK_GPU(t);
    TORCH_CHECK(w1.scalar_type() == at::kBFloat16,
                "timestep_embed_mlp: bf16 weight");
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
        b1c = b1->contiguous();
        TORCH_CHECK(b1c.scalar_type() == at::kBFloat16 &&
                    (int)b1c.numel() == H, "timestep_embed_mlp: bias [H] bf16");
        bias = (const bf16*)b1c.data_ptr();
    }
    const int hblocks = (H + 255) / 256;
    hipLaunchKernelGGL(ts_embed_mlp_kernel, dim3(B * hblocks), dim3(256),
                       K * sizeof(float), cur_stream(), tc.data_ptr<float>(),
                       (const bf16*)w1c.data_ptr(), bias,
                       (bf16*)out.data_ptr(), H, K, (float)max_period,
                       (float)time_factor);
    return out;
}


void qk_norm_rope_(at::Tensor q, at::Tensor k, at::Tensor wq, at::Tensor wk,
                   at::Tensor cs, double eps) {
    CHECK_GPU(q);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "qk_norm_rope_: [B,S,H,D] views");
    TORCH_CHECK(is_elem16(q.scalar_type()),
                "qk_norm_rope_: bf16 or fp16 only, got ", q.scalar_type());
    CHECK_SAME_DTYPE(k, q);
    CHECK_SAME_DTYPE(wq, q);
    CHECK_SAME_DTYPE(wk, q);
    TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1, "last dim contiguous");
    const int B = (int)q.size(0), S = (int)q.size(1), H = (int)q.size(2),
              D = (int)q.size(3);
    TORCH_CHECK(D % 2 == 0 && D <= 128, "qk_norm_rope_: D must be even, <=128");
    TORCH_CHECK((int)k.size(1) == S && (int)k.size(2) == H, "k shape mismatch");
    auto csf = cs.to(at::kFloat).contiguous();
    TORCH_CHECK((int)csf.size(0) == S && (int)csf.size(1) == D / 2, "cs shape");
    auto wqc = wq.contiguous();
    auto wkc = wk.contiguous();
    const long rows = (long)B * S * H;
    const long blocks = (((rows + 3) / 4) * 64 + 255) / 256;
    PA_WITH_ELEM16(q.scalar_type(), hipLaunchKernelGGL(
        qk_norm_rope_kernel<E>, dim3((unsigned)blocks), dim3(256), 0,
        cur_stream(), (E*)q.data_ptr(), (E*)k.data_ptr(),
        (const E*)wqc.data_ptr(), (const E*)wkc.data_ptr(),
        csf.data_ptr<float>(), S, H, D,
        q.stride(0), q.stride(2), q.stride(1),
        k.stride(0), k.stride(2), k.stride(1), rows, (float)eps));
}



// ---------------------------------------------------------------------------
// Fused joint-qkv pack for dual-stream MMDiT blocks: reads the txt and img
// qkv projection buffers (strided [B,S,3,H,D] views), applies per-stream qk
// RMSNorm + RoPE, and writes CONTIGUOUS joint q/k/v [B, T+Si, H, D] —
// replacing three strided torch.cat copies plus two qk_norm_rope passes
// with a single bandwidth pass. One wave per (b, s, h); lane = pair index.
// ---------------------------------------------------------------------------
template <typename E>
__global__ void pack_joint_qkv_kernel(
    const E* __restrict__ txt, const E* __restrict__ img,
    const E* __restrict__ wq_t, const E* __restrict__ wk_t,
    const E* __restrict__ wq_i, const E* __restrict__ wk_i,
    const float* __restrict__ cs,                   // [T+Si][D/2][2]
    E* __restrict__ oq, E* __restrict__ ok, E* __restrict__ ov,
    int T, int Si, int H, int D,
    long t_bs, long t_ss, long t_qs, long t_hs,     // txt strides (b, s, qkv, h)
    long i_bs, long i_ss, long i_qs, long i_hs,
    long n_rows, float eps) {
    // RPW rows per wave, all 3*RPW loads issued before the reductions
    // (single-row version measured latency-bound like qk_norm_rope).
    using EL = Elem16<E>;
    constexpr int RPW = 4;
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int S = T + Si;
    const int pairs = D / 2;
    // Same D<128 rule as qk_norm_rope_kernel: lanes >= pairs stay alive for
    // the 64-lane reductions (contributing 0), load clamped, never store.
    const bool act = lane < pairs;
    const int ln = act ? lane : 0;

    unsigned int uq[RPW], uk[RPW], uv[RPW], uwq[RPW], uwk[RPW];
    long obase[RPW];
    float cvec[RPW], svec[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const long row = wave * RPW + i;
        const long rr = row < n_rows ? row : n_rows - 1;
        const long b = rr / ((long)S * H);
        const long sh = rr % ((long)S * H);
        const int sj = (int)(sh / H);
        const int h = (int)(sh % H);
        const bool is_txt = sj < T;
        const E* src = is_txt
            ? txt + b * t_bs + (long)sj * t_ss + (long)h * t_hs
            : img + b * i_bs + (long)(sj - T) * i_ss + (long)h * i_hs;
        const long qs = is_txt ? t_qs : i_qs;
        uq[i] = reinterpret_cast<const unsigned int*>(src)[ln];
        uk[i] = reinterpret_cast<const unsigned int*>(src + qs)[ln];
        uv[i] = reinterpret_cast<const unsigned int*>(src + 2 * qs)[ln];
        uwq[i] = reinterpret_cast<const unsigned int*>(is_txt ? wq_t : wq_i)[ln];
        uwk[i] = reinterpret_cast<const unsigned int*>(is_txt ? wk_t : wk_i)[ln];
        cvec[i] = cs[((long)sj * pairs + ln) * 2 + 0];
        svec[i] = cs[((long)sj * pairs + ln) * 2 + 1];
        obase[i] = (((long)b * S + sj) * H + h) * (D / 2);
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        if (wave * RPW + i >= n_rows) break;
        const float c = cvec[i], sn = svec[i];
        {   // q: rms + weight + rope
            float a0 = EL::ld((unsigned short)(uq[i] & 0xffff));
            float a1 = EL::ld((unsigned short)(uq[i] >> 16));
            float ss_ = act ? a0 * a0 + a1 * a1 : 0.f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) ss_ += __shfl_xor(ss_, off, 64);
            const float rr = rsqrtf(ss_ / (float)D + eps);
            a0 = a0 * rr * EL::ld((unsigned short)(uwq[i] & 0xffff));
            a1 = a1 * rr * EL::ld((unsigned short)(uwq[i] >> 16));
            if (act)
                reinterpret_cast<unsigned int*>(oq)[obase[i] + lane] =
                    (unsigned int)EL::st(a0 * c - a1 * sn) |
                    ((unsigned int)EL::st(a0 * sn + a1 * c) << 16);
        }
        {   // k
            float a0 = EL::ld((unsigned short)(uk[i] & 0xffff));
            float a1 = EL::ld((unsigned short)(uk[i] >> 16));
            float ss_ = act ? a0 * a0 + a1 * a1 : 0.f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) ss_ += __shfl_xor(ss_, off, 64);
            const float rr = rsqrtf(ss_ / (float)D + eps);
            a0 = a0 * rr * EL::ld((unsigned short)(uwk[i] & 0xffff));
            a1 = a1 * rr * EL::ld((unsigned short)(uwk[i] >> 16));
            if (act)
                reinterpret_cast<unsigned int*>(ok)[obase[i] + lane] =
                    (unsigned int)EL::st(a0 * c - a1 * sn) |
                    ((unsigned int)EL::st(a0 * sn + a1 * c) << 16);
        }
        if (act) reinterpret_cast<unsigned int*>(ov)[obase[i] + lane] = uv[i];
    }
}

// Half-wave exchange without LDS: combine x with the partner lane's x
// (lane i <-> lane i^32). v_permlane32_swap trades the upper half of its
// first operand for the lower half of its second, so of the two results one
// is this lane's own x and the other its partner's; which is which depends
// on the half, and a commutative f gives both lanes the same bits. A VALU
// op: no ds_bpermute round trip and no lgkmcnt wait in the caller's chain.
template <typename F>
PA_DEV float half_swap_combine(float x, F f) {
    const unsigned int u = __float_as_uint(x);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return f(__uint_as_float((unsigned int)r[0]),
             __uint_as_float((unsigned int)r[1]));
}
// One v_mul_f32 that the SLP vectorizer cannot pair into v_pk_mul_f32
// (packed f32 VALU beside MFMAs costs more than the two scalar ops).
PA_DEV float mul_f32_scalar(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ---------------------------------------------------------------------------
// Attention v4: swapped-QK^T 32x32 structure (guide Appendix B ladder).
//
// mfma_f32_32x32x16_bf16 computing S^T = K·Q^T, so each LANE owns a full
// query ROW: softmax max/sum are a 32-value local reduce + ONE half-wave
// exchange with the partner lane (half_swap_combine, no LDS); running (m, l)
// and the per-tile O-rescale are lane-local scalars. P converts f32->bf16
// in-register
// (v_cvt_pk_bf16_f32) and redistributes across half-waves with
// v_permlane32_swap (T12) — NO P staging through LDS. PV computes
// O^T = V^T · P^T (same P fragments serve as the B operand), keeping the
// output row lane-local for the rescale and the 1/l epilogue.
//
// V operand via gfx950's ds_read_b64_tr_b16 hardware transpose-read (guide
// T10): V is stored ROW-major ([key][dim], plain b128 stores straight from
// the HBM staging registers — no per-element transpose pass) with a
// 40-granule (160-element) row stride, which is ≡ 8 (mod 32) so each
// tr-read cycle hits 32 distinct banks, plus a (key&8)<<1 column XOR that
// keeps the two wave halves bank-disjoint. PV A-fragments are gathered by
// two tr reads per (chunk, tile) from one base VGPR + immediate offsets.
// Gather semantics verified empirically (scripts/tr_probe.hip): within a
// 16-lane group, lane L reg j = element (L&3) of the granule addressed by
// lane (L>>2)+4j. Measured +9.3% flux / +7.4% long-S over the swizzled
// scalar-store image (scripts/attn_ab.hip, within-probe interleaved).
//
// Geometry: 512-thread blocks (8 waves x 32 q-rows = 256 rows/block);
// LDS = K[64][D+8] + row-major V[64][160] = 37.9 KB (D=128) -> two blocks
// co-resident per CU, NOT barrier-synced against each other.
// ---------------------------------------------------------------------------
// The element type E (bf16 or _Float16) enters at three points only: the
// MFMA opcode, the P pack (Elem16<E>::pack2) and the epilogue cast. Every
// LDS layout, tr read and permlane swap is a 16-bit move and is shared;
// the mask sentinel, online-softmax state and accumulators stay fp32.
//
// MASKED (key-padding mask, see pack_key_mask_kernel): the KV loop walks the
// batch element's compacted list of live tiles instead of 0..n_tiles-1, and
// the per-key validity test `key < Sk` becomes that key's bit in the tile's
// 64-bit mask word (bits at or beyond Sk are 0, so the bit implies the
// bound). A dead tile is never loaded or multiplied — the -1e30/-3e30
// sentinel arithmetic relies on every processed tile holding at least one
// live key — and a masked K/V row is staged as zeros, so its contents are
// don't-care. nlive == 0 skips the loop (prologue included) and the
// epilogue's inv_l = 0 writes zeros. Both variants run the same KV loops
// (see "KV loop" in the body); `if constexpr (MASKED)` only picks where the
// trip count, the tile index and the mask word come from, and the unmasked
// instantiations compile to the code they had before the flag existed.
template <int D, typename E, bool MASKED = false>
__global__ __launch_bounds__(512, 2) void attn_fwd_v4_kernel(
    const E* __restrict__ q, const E* __restrict__ k,
    const E* __restrict__ v, E* __restrict__ out,
    int S, int Sk, float scale, int H,
    long q_bs, long q_hs, int q_ss,
    long k_bs, long k_hs, int k_ss,
    long v_bs, long v_hs, int v_ss,
    long o_bs, long o_hs, int o_ss, int xcd_grid,
    E* __restrict__ out2, int s_split,
    long o2_bs, long o2_hs, int o2_ss,
    const unsigned long long* __restrict__ mask_words = nullptr,
    const int* __restrict__ mask_live = nullptr,
    const int* __restrict__ mask_nlive = nullptr) {
    using EL = Elem16<E>;
    constexpr int KVBLK = 64;
    constexpr int WAVES = 8;
    constexpr int THREADS = WAVES * 64;
    constexpr int KPAD = D + 8;
    constexpr int VROW = 160;        // V row stride: 40 granules ≡ 8 mod 32
    constexpr int KK = D / 16;        // QK^T K-steps per 32-key tile
    constexpr int NV = D / 32;        // PV dim tiles
    constexpr int KVECS = (KVBLK * D) / (8 * THREADS);
    // D=128: double-buffered LDS (75.8 KB, still 2 blocks/CU) for the v5a
    // 1-barrier pipelined schedule; D=64 keeps the v4 2-barrier loop.
    constexpr int DBUF = (D == 128) ? 2 : 1;

    __shared__ E k_lds[DBUF * KVBLK * KPAD];
    __shared__ E v_lds[DBUF * KVBLK * VROW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l32 = lane & 31;        // this lane's query row (within wave)
    const int hi = lane >> 5;         // half-wave id
    // tr_b16 per-lane base: this lane supplies the granule
    // (key = hi*8 + (p>>2) [+16c+4rd], col = 32n + 16*((G&1)^hi) + 4*(p&3))
    const int trb = (hi * 8 + ((lane & 15) >> 2)) * VROW +
                    16 * (((lane >> 4) & 1) ^ hi) + 4 * (lane & 3);

    long bh;
    int qtile;
    if (xcd_grid) {
        // XCD-affine decode: xcd = id%8, bh = xcd + 8*(id/8 / nq),
        // qtile = (id/8) % nq  (bijective when BH % 8 == 0)
        const int nq = (S + WAVES * 32 - 1) / (WAVES * 32);
        const long id = blockIdx.x;
        const long xcd = id & 7;
        const long within = id >> 3;
        bh = xcd + 8 * (within / nq);
        qtile = (int)(within % nq);
    } else {
        bh = blockIdx.y;
        qtile = blockIdx.x;
    }
    const long b = bh / H;
    const int h = (int)(bh % H);
    const int q0 = qtile * (WAVES * 32) + wid * 32;

    const E* qp = q + b * q_bs + (long)h * q_hs;
    const E* kp = k + b * k_bs + (long)h * k_hs;
    const E* vp = v + b * v_bs + (long)h * v_hs;
    E* op = out + b * o_bs + (long)h * o_hs;
    E* op2 = out2 ? out2 + b * o2_bs + (long)h * o2_hs : nullptr;

    // Q fragments (B-operand of the swapped QK^T): lane holds
    // Q[q0 + l32][kk*16 + hi*8 + j], j = 0..7.
    bf16x8 qfrag[KK];
    {
        const int row = q0 + l32;
        const int rr = row < S ? row : (S > 0 ? S - 1 : 0);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
            qfrag[kk] = *reinterpret_cast<const bf16x8*>(
                qp + (long)rr * q_ss + kk * 16 + hi * 8);
    }

    f32x16 o_acc[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[n][r] = 0.f;
    float m_run = -1e30f, l_run = 0.f;
    const float scale2 = scale * PA_LOG2E;

    bf16x8 kreg[KVECS], vreg[KVECS];
    // `word` (MASKED only) is the tile's mask word: bit `row` set = stage
    // the row, clear = stage zeros (covers src >= Sk, whose bits are 0)
    auto issue_tile_loads = [&](int kv0, unsigned long long word = 0) {
#pragma unroll
        for (int i = 0; i < KVECS; ++i) {
            const int idx = tid + i * THREADS;
            const int row = idx / (D / 8);
            const int col = (idx % (D / 8)) * 8;
            const int src = kv0 + row;
            bool stage;
            if constexpr (MASKED) stage = ((word >> row) & 1ull) != 0;
            else stage = src < Sk;
            if (stage) {
                kreg[i] = *reinterpret_cast<const bf16x8*>(kp + (long)src * k_ss + col);
                vreg[i] = *reinterpret_cast<const bf16x8*>(vp + (long)src * v_ss + col);
            } else {
                kreg[i] = bf16x8{0,0,0,0,0,0,0,0};
                vreg[i] = bf16x8{0,0,0,0,0,0,0,0};
            }
        }
    };
    auto write_k_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < KVECS; ++i) {
            const int idx = tid + i * THREADS;
            const int row = idx / (D / 8);
            const int col = (idx % (D / 8)) * 8;
            *reinterpret_cast<bf16x8*>(
                &k_lds[buf * (KVBLK * KPAD) + row * KPAD + col]) = kreg[i];
        }
    };
    auto write_v_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < KVECS; ++i) {
            const int idx = tid + i * THREADS;
            const int row = idx / (D / 8);
            const int col = (idx % (D / 8)) * 8;
            // row-major V, b128 store; column XOR by (row&8)<<1 keeps the
            // tr gather conflict-free under either half-wave pairing
            *reinterpret_cast<bf16x8*>(
                &v_lds[buf * (KVBLK * VROW) + row * VROW +
                       (col ^ ((row & 8) << 1))]) = vreg[i];
        }
    };

    // ---- per-tile phases --------------------------------------------------
    auto qk_phase = [&](int buf, f32x16* st) {
        // swapped QK^T: S^T[key][row] for two 32-key tiles;
        // A = K chunk: lane holds K[kt*32 + l32][kk*16 + hi*8 + j]
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[kt][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                bf16x8 afrag = *reinterpret_cast<const bf16x8*>(
                    &k_lds[buf * (KVBLK * KPAD) + (kt * 32 + l32) * KPAD +
                           kk * 16 + hi * 8]);
                st[kt] = EL::mfma32(afrag, qfrag[kk], st[kt]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };
    auto softmax_phase = [&](int kv0, f32x16* st, bf16x8* pfrag,
                             unsigned long long word = 0) {
        // lane-local online softmax (this lane's row = q0 + l32);
        // value (kt, reg) = S[row][key = kt*32 + (reg&3) + 8*(reg>>2) + 4*hi]
        // raw tile max (scale2 > 0 commutes with max), softmax scale fused
        // into the exp2 argument as one FMA per element.
        //
        // Per-key validity only where a tile can hold a dead key: `full` is
        // block-uniform (Sk and kv0 are scalars, the mask word is pinned in
        // SGPRs), so a full tile branches over the whole substitution — no
        // key index, compare or select — and uses the scores as qk_phase
        // left them. Every tile of an Sk % 64 == 0 call is full. The
        // substitution works in place ahead of ONE softmax body: a second,
        // compile-time-full copy of the body costs registers (D=128 spills,
        // D=64 loses a resident block; scripts/attn_v6.hip v4/v5).
        bool full;
        if constexpr (MASKED) full = word == ~0ull;
        else full = kv0 + KVBLK <= Sk;
        if (!full) {
            // MASKED: this lane's keys are bits 4*hi + (r&3) + 8*(r>>2) of
            // the word's half kt — one 64-bit shift, then constant bit
            // positions
            unsigned int wh[2] = {0u, 0u};
            if constexpr (MASKED) {
                const unsigned long long wl = word >> (4 * hi);
                wh[0] = (unsigned int)wl;
                wh[1] = (unsigned int)(wl >> 32);
            }
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key =
                        kv0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    bool valid;
                    if constexpr (MASKED)
                        valid =
                            ((wh[kt] >> ((r & 3) + 8 * (r >> 2))) & 1u) != 0;
                    else
                        valid = key < Sk;
                    st[kt][r] = valid ? st[kt][r] : -3e30f;
                }
        }
        float mx = -3e30f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[kt][r]);
        // partner: row's other 32 keys
        mx = half_swap_combine(
            mx, [](float a, float c) { return fmaxf(a, c); });
        const float mnew = fmaxf(m_run, mx * scale2);
        const float alpha = __builtin_amdgcn_exp2f(m_run - mnew);
        m_run = mnew;
        float ps = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv_ =
                    __builtin_amdgcn_exp2f(fmaf(st[kt][r], scale2, -mnew));
                st[kt][r] = pv_;
                ps += pv_;
            }
        ps = half_swap_combine(ps, [](float a, float c) { return a + c; });
        l_run = l_run * alpha + ps;
        if (alpha != 1.f) {
            // D=128: 64 scalar v_mul_f32; left to the compiler they become
            // 32 v_pk_mul_f32, slower beside the MFMAs there. D=64 measured
            // the other way round and keeps the packed form
            // (scripts/attn_v6.hip, v3 against v2).
#pragma unroll
            for (int n = 0; n < NV; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (D == 128)
                        o_acc[n][r] = mul_f32_scalar(o_acc[n][r], alpha);
                    else
                        o_acc[n][r] *= alpha;
                }
        }
        // P f32 -> 16-bit fragments via cvt_pk + permlane32_swap: chunk c
        // (16 keys) uses regs 8*(c&1)..+7 of st[c>>1]; after the half-swap
        // each lane holds P[row l32][chunk base + hi*8 + j].
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x16& sv = st[c >> 1];
            const int rb = 8 * (c & 1);
            unsigned int w0 = EL::pack2(sv[rb + 0], sv[rb + 1]);
            unsigned int w1 = EL::pack2(sv[rb + 2], sv[rb + 3]);
            unsigned int w2 = EL::pack2(sv[rb + 4], sv[rb + 5]);
            unsigned int w3 = EL::pack2(sv[rb + 6], sv[rb + 7]);
            auto r02 = __builtin_amdgcn_permlane32_swap(w0, w2, false, false);
            auto r13 = __builtin_amdgcn_permlane32_swap(w1, w3, false, false);
            unsigned int d[4] = {(unsigned int)r02[0], (unsigned int)r13[0],
                                 (unsigned int)r02[1], (unsigned int)r13[1]};
            pfrag[c] = *reinterpret_cast<bf16x8*>(d);
        }
    };
    auto pv_phase = [&](int buf, bf16x8* pfrag) {
        // PV: O^T[dim][row] += V^T chunk · P^T chunk; A = V^T gathered from
        // the row-major V image by ds_read_b64_tr_b16 (2 reads per (c, n)).
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int n = 0; n < NV; ++n) {
                short4v alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) short4v*)
                        &v_lds[buf * (KVBLK * VROW) + trb + c * (16 * VROW) +
                               n * 32]);
                short4v ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) short4v*)
                        &v_lds[buf * (KVBLK * VROW) + trb + c * (16 * VROW) +
                               4 * VROW + n * 32]);
                bf16x8 va = __builtin_shufflevector(alo, ahi,
                                                    0, 1, 2, 3, 4, 5, 6, 7);
                o_acc[n] = EL::mfma32(va, pfrag[c], o_acc[n]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };

    // ---- KV loop ----------------------------------------------------------
    // One loop per schedule, written over three block-uniform accessors so
    // the masked and unmasked instantiations share it:
    //   nt          trip count: nlive[b] (MASKED) or n_tiles
    //   tile_at(j)  j-th tile to process: live[b][j] (MASKED) or j
    //   word_of(t)  tile t's 64-bit mask word (MASKED) or 0 (ignored)
    // b is uniform across the block, so are nt, every tile index and every
    // mask word: readfirstlane pins them in SGPRs, and trip counts and
    // barriers stay block-uniform. With MASKED, nt == 0 skips the prologue's
    // loads, LDS writes and barrier too; the unmasked prologue is
    // unconditional, as it was before the flag existed.
    const int n_tiles = (Sk + KVBLK - 1) / KVBLK;
    const int* live_b = MASKED ? mask_live + b * n_tiles : nullptr;
    const unsigned long long* words_b =
        MASKED ? mask_words + b * n_tiles : nullptr;
    const int nt =
        MASKED ? __builtin_amdgcn_readfirstlane(mask_nlive[b]) : n_tiles;
    auto tile_at = [&](int j) {
        if constexpr (MASKED)
            return __builtin_amdgcn_readfirstlane(live_b[j]);
        else
            return j;
    };
    auto word_of = [&](int tile) -> unsigned long long {
        if constexpr (MASKED) {
            const unsigned long long w = words_b[tile];
            const unsigned int lo =
                __builtin_amdgcn_readfirstlane((unsigned int)w);
            const unsigned int hi32 =
                __builtin_amdgcn_readfirstlane((unsigned int)(w >> 32));
            return ((unsigned long long)hi32 << 32) | lo;
        } else {
            return 0ull;
        }
    };
    // (the loads are written out at each site: wrapping tile_at + word_of +
    // issue_tile_loads in one more lambda reorders the unmasked code)
    if constexpr (DBUF == 2) {
        // v5a pipelined schedule (measured +4.0% flux / +4.2% long-S over
        // the 2-barrier loop, scripts/attn_v5.hip): double-buffered LDS,
        // ONE barrier per tile; tile j+1's stores land in the other buffer
        // interleaved where the LDS port is idle (K after QK^T, V after
        // softmax); tile j+2's global loads issue before PV.
        if (!MASKED || nt > 0) {
            const int t0 = tile_at(0);
            issue_tile_loads(t0 * KVBLK, word_of(t0));
            write_k_lds(0);
            write_v_lds(0);
            if (nt > 1) {
                const int t1 = tile_at(1);
                issue_tile_loads(t1 * KVBLK, word_of(t1));
            }
            __syncthreads();
        }
        for (int j = 0; j < nt; ++j) {
            const int p = j & 1;
            const int tile = tile_at(j);
            f32x16 st[2];
            bf16x8 pfrag[4];
            qk_phase(p, st);
            if (j + 1 < nt) write_k_lds(p ^ 1);
            softmax_phase(tile * KVBLK, st, pfrag, word_of(tile));
            if (j + 1 < nt) write_v_lds(p ^ 1);
            if (j + 2 < nt) {
                const int t2 = tile_at(j + 2);
                issue_tile_loads(t2 * KVBLK, word_of(t2));
            }
            pv_phase(p, pfrag);
            __syncthreads();
        }
    } else {
        // D=64 keeps the v4 2-barrier loop (v5a measured -2.6% there —
        // halved MFMA per tile leaves too little compute to hide stores).
        if (!MASKED || nt > 0) {
            const int t0 = tile_at(0);
            issue_tile_loads(t0 * KVBLK, word_of(t0));
        }
        for (int j = 0; j < nt; ++j) {
            const int tile = tile_at(j);
            __syncthreads();
            write_k_lds(0);
            write_v_lds(0);
            __syncthreads();
            if (j + 1 < nt) {
                const int t1 = tile_at(j + 1);
                issue_tile_loads(t1 * KVBLK, word_of(t1));
            }
            f32x16 st[2];
            bf16x8 pfrag[4];
            qk_phase(0, st);
            softmax_phase(tile * KVBLK, st, pfrag, word_of(tile));
            pv_phase(0, pfrag);
        }
    }

    // ---- epilogue: O = O^T / l, row is lane-local -------------------------
    const int row = q0 + l32;
    if (row < S) {
        // split-stream output: rows >= s_split land in out2 (per-stream
        // contiguous buffers feed the txt/img projections with no reshape
        // copies)
        E* obase;
        long orow;
        int oss;
        if (op2 != nullptr && row >= s_split) {
            obase = op2;
            orow = row - s_split;
            oss = o2_ss;
        } else {
            obase = op;
            orow = row;
            oss = o_ss;
        }
        const float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
        for (int n = 0; n < NV; ++n) {
#pragma unroll
            for (int r2 = 0; r2 < 4; ++r2) {
                // dims n*32 + 8*r2 + 4*hi + (0..3) are consecutive
                const int dim0 = n * 32 + 8 * r2 + 4 * hi;
                unsigned short pack[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    pack[j] = EL::st(o_acc[n][r2 * 4 + j] * inv_l);
                *reinterpret_cast<unsigned long long*>(
                    obase + orow * oss + dim0) =
                    *reinterpret_cast<unsigned long long*>(pack);
            }
        }
    }
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
    const int blocks = (int)std::min<long>((total8 + 255) / 256, 4096);
    hipLaunchKernelGGL(gelu_fp8_kernel, dim3(blocks), dim3(256), 0,
                       cur_stream(), (const bf16*)xc.data_ptr(),
                       (unsigned char*)out.data_ptr(), total8,
                       scale.data_ptr<float>(), amax_buf.data_ptr<float>());
    fp8_scale_finalize(scale, amax_buf, scale_used);
    return out;
}

at::Tensor gelu_tanh(at::Tensor x) {
    CHECK_GPU(x);
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
    if (is_elem16(x.scalar_type()) && rowable && (w % 8) == 0 &&
        (in_stride % 8) == 0) {
        auto out = at::empty(x.sizes(), x.options());
        const long total8 = rows * (w / 8);
        const int blocks = (int)std::min<long>((total8 + 255) / 256, 4096);
        PA_WITH_ELEM16(x.scalar_type(), hipLaunchKernelGGL(
            gelu_tanh_vec_kernel<E>, dim3(blocks), dim3(256), 0,
            cur_stream(), (const E*)x.data_ptr(), (E*)out.data_ptr(),
            total8, rows, w / 8, in_stride / 8));
        return out;
    }
    auto xc = x.contiguous();
    auto out = at::empty_like(xc);
    if (is_elem16(xc.scalar_type()) && (xc.numel() % 8) == 0) {
        const long total8 = xc.numel() / 8;
        const int blocks = (int)std::min<long>((total8 + 255) / 256, 4096);
        PA_WITH_ELEM16(xc.scalar_type(), hipLaunchKernelGGL(
            gelu_tanh_vec_kernel<E>, dim3(blocks), dim3(256), 0,
            cur_stream(), (const E*)xc.data_ptr(), (E*)out.data_ptr(),
            total8, xc.numel() / 8, xc.numel() / 8, xc.numel() / 8));
        return out;
    }
    return at::gelu(xc, "tanh");
}


std::vector<at::Tensor> pack_joint_qkv(at::Tensor txt_qkv, at::Tensor img_qkv,
                                       at::Tensor wq_t, at::Tensor wk_t,
                                       at::Tensor wq_i, at::Tensor wk_i,
                                       at::Tensor cs, double eps) {
    CHECK_GPU(txt_qkv);
    TORCH_CHECK(txt_qkv.dim() == 5 && img_qkv.dim() == 5,
                "pack_joint_qkv expects [B,S,3,H,D] views");
    TORCH_CHECK(is_elem16(txt_qkv.scalar_type()),
                "pack_joint_qkv: bf16 or fp16 only, got ",
                txt_qkv.scalar_type());
    CHECK_SAME_DTYPE(img_qkv, txt_qkv);
    CHECK_SAME_DTYPE(wq_t, txt_qkv);
    CHECK_SAME_DTYPE(wk_t, txt_qkv);
    CHECK_SAME_DTYPE(wq_i, txt_qkv);
    CHECK_SAME_DTYPE(wk_i, txt_qkv);
    const int B = (int)txt_qkv.size(0), T = (int)txt_qkv.size(1),
              H = (int)txt_qkv.size(3), D = (int)txt_qkv.size(4);
    const int Si = (int)img_qkv.size(1);
    TORCH_CHECK(txt_qkv.stride(4) == 1 && img_qkv.stride(4) == 1,
                "last dim contiguous");
    TORCH_CHECK(D % 2 == 0 && D <= 128, "D must be even and <= 128");
    auto csf = cs.to(at::kFloat).contiguous();
    TORCH_CHECK((int)csf.size(0) == T + Si, "cs must cover the joint sequence");
    auto opts = txt_qkv.options();
    auto oq = at::empty({B, T + Si, H, D}, opts);
    auto ok = at::empty({B, T + Si, H, D}, opts);
    auto ov = at::empty({B, T + Si, H, D}, opts);
    const long rows = (long)B * (T + Si) * H;
    const long blocks = (((rows + 3) / 4) * 64 + 255) / 256;
    auto wqtc = wq_t.contiguous(), wktc = wk_t.contiguous();
    auto wqic = wq_i.contiguous(), wkic = wk_i.contiguous();
    PA_WITH_ELEM16(txt_qkv.scalar_type(), hipLaunchKernelGGL(
        pack_joint_qkv_kernel<E>, dim3((unsigned)blocks), dim3(256),
        0, cur_stream(),
        (const E*)txt_qkv.data_ptr(), (const E*)img_qkv.data_ptr(),
        (const E*)wqtc.data_ptr(), (const E*)wktc.data_ptr(),
        (const E*)wqic.data_ptr(), (const E*)wkic.data_ptr(),
        csf.data_ptr<float>(),
        (E*)oq.data_ptr(), (E*)ok.data_ptr(), (E*)ov.data_ptr(),
        T, Si, H, D,
        txt_qkv.stride(0), txt_qkv.stride(1), txt_qkv.stride(2),
        txt_qkv.stride(3),
        img_qkv.stride(0), img_qkv.stride(1), img_qkv.stride(2),
        img_qkv.stride(3),
        rows, (float)eps));
    return {oq, ok, ov};
}


at::Tensor quant_fp8(at::Tensor x, at::Tensor scale, at::Tensor amax_buf,
                     at::Tensor scale_used) {
    CHECK_GPU(x);
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, "quant_fp8: bf16 input");
    auto xc = x.contiguous();
    TORCH_CHECK((xc.numel() % 8) == 0, "quant_fp8: numel % 8 == 0");
    auto out = at::empty(xc.sizes(), xc.options().dtype(at::kFloat8_e4m3fn));
    const long total8 = xc.numel() / 8;
    const int blocks = (int)std::min<long>((total8 + 255) / 256, 4096);
    hipLaunchKernelGGL(quant_fp8_bf16_kernel, dim3(blocks), dim3(256), 0,
                       cur_stream(), (const bf16*)xc.data_ptr(),
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

// ---------------------------------------------------------------------------
// Key-padding mask pack: [B, Sk] bool (nonzero = attend) -> what the MASKED
// attention instantiations read.
//   words[b][t]  bit j = mask[b][64*t + j]; bits at or beyond Sk are 0
//   live[b][..]  ascending indices of tiles with a nonzero word, compacted
//                to the front (the tail is zero-filled)
//   nlive[b]     how many
// One 256-thread block per batch element (launch-bound, not bandwidth-
// bound): every wave ballots 64 keys per step into the word, then wave 0
// compacts 64 tiles per step with a ballot + prefix popcount. Everything
// stays on the device, so the op is graph-capturable.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_key_mask_kernel(
    const unsigned char* __restrict__ mask, unsigned long long* words,
    int* __restrict__ live, int* __restrict__ nlive, int Sk, int n_tiles) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const unsigned char* mb = mask + (long)b * Sk;
    unsigned long long* wb = words + (long)b * n_tiles;
    int* lb = live + (long)b * n_tiles;
    for (int t = wid; t < n_tiles; t += 4) {
        const int key = t * 64 + lane;
        const bool on = key < Sk && mb[key] != 0;
        const unsigned long long w = __ballot(on);
        if (lane == 0) wb[t] = w;
    }
    __syncthreads();  // words of this batch element visible to wave 0
    if (wid != 0) return;
    int count = 0;
    for (int base = 0; base < n_tiles; base += 64) {
        const int t = base + lane;
        const bool alive = t < n_tiles && wb[t] != 0ull;
        const unsigned long long m = __ballot(alive);
        if (alive)
            lb[count + __popcll(m & ((1ull << lane) - 1ull))] = t;
        count += __popcll(m);
    }
    for (int i = count + lane; i < n_tiles; i += 64) lb[i] = 0;
    if (lane == 0) nlive[b] = count;
}

std::vector<at::Tensor> pack_key_mask(at::Tensor mask) {
    CHECK_GPU(mask);
    TORCH_CHECK(mask.dim() == 2, "pack_key_mask expects a [B, Sk] mask");
    TORCH_CHECK(mask.scalar_type() == at::kBool ||
                    at::isIntegralType(mask.scalar_type(), false),
                "pack_key_mask: bool or integer mask only (nonzero = attend); "
                "additive float biases are not supported, got ",
                mask.scalar_type());
    // integer masks: nonzero -> true, on the device (no host read)
    auto mb = (mask.scalar_type() == at::kBool ? mask : mask.ne(0))
                  .contiguous();
    const int B = (int)mb.size(0), Sk = (int)mb.size(1);
    const int n_tiles = (Sk + 63) / 64;
    auto words = at::empty({B, n_tiles}, mb.options().dtype(at::kLong));
    auto live = at::empty({B, n_tiles}, mb.options().dtype(at::kInt));
    auto nlive = at::empty({B}, mb.options().dtype(at::kInt));
    if (B > 0)
        hipLaunchKernelGGL(pack_key_mask_kernel, dim3((unsigned)B), dim3(256),
                           0, cur_stream(),
                           (const unsigned char*)mb.data_ptr(),
                           (unsigned long long*)words.data_ptr(),
                           live.data_ptr<int>(), nlive.data_ptr<int>(), Sk,
                           n_tiles);
    return {words, live, nlive};
}

// Packed key mask as the MASKED kernels take it (see pack_key_mask).
struct AttnKeyMask {
    at::Tensor words, live, nlive;
};

// Arguments of one attention launch, in the kernels' parameter order
// (attn_fwd_kernel takes the first twenty). Pointers are untyped here; the
// launch casts them to the element type.
struct AttnArgs {
    const void *q, *k, *v;
    void* out;
    int S, Sk;
    float scale;
    int H;
    long q_bs, q_hs;
    int q_ss;
    long k_bs, k_hs;
    int k_ss;
    long v_bs, v_hs;
    int v_ss;
    long o_bs, o_hs;
    int o_ss, xcd_grid;
    void* out2;
    int s_split;
    long o2_bs, o2_hs;
    int o2_ss;
    const unsigned long long* mask_words;
    const int *mask_live, *mask_nlive;
};

template <int D, bool MASKED>
static void launch_attn_v4(at::ScalarType st, dim3 grid, const AttnArgs& a) {
    PA_WITH_ELEM16(st, hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_fwd_v4_kernel<D, E, MASKED>), grid, dim3(512), 0,
        cur_stream(), (const E*)a.q, (const E*)a.k, (const E*)a.v, (E*)a.out,
        a.S, a.Sk, a.scale, a.H, a.q_bs, a.q_hs, a.q_ss, a.k_bs, a.k_hs,
        a.k_ss, a.v_bs, a.v_hs, a.v_ss, a.o_bs, a.o_hs, a.o_ss, a.xcd_grid,
        (E*)a.out2, a.s_split, a.o2_bs, a.o2_hs, a.o2_ss, a.mask_words,
        a.mask_live, a.mask_nlive));
}

// PA_ATTN_V3=1: the previous-generation bf16 debug kernel.
template <int D>
static void launch_attn_v3(dim3 grid, const AttnArgs& a) {
    hipLaunchKernelGGL(
        attn_fwd_kernel<D>, grid, dim3(512), 0, cur_stream(),
        (const bf16*)a.q, (const bf16*)a.k, (const bf16*)a.v, (bf16*)a.out,
        a.S, a.Sk, a.scale, a.H, a.q_bs, a.q_hs, a.q_ss, a.k_bs, a.k_hs,
        a.k_ss, a.v_bs, a.v_hs, a.v_ss, a.o_bs, a.o_hs, a.o_ss);
}

// The one attention launcher. split > 0 (bshd only) writes rows >= split to
// a second tensor; km != nullptr selects the MASKED instantiations.
static std::vector<at::Tensor> attn_fwd_launch(
    at::Tensor q, at::Tensor k, at::Tensor v, double scale, bool bshd,
    long split, const AttnKeyMask* km) {
    CHECK_GPU(q);
    TORCH_CHECK(is_elem16(q.scalar_type()),
                "attn_fwd: bf16 or fp16 only, got ", q.scalar_type());
    CHECK_SAME_DTYPE(k, q);
    CHECK_SAME_DTYPE(v, q);
    TORCH_CHECK(q.dim() == 4, "attn_fwd expects 4-D q/k/v");
    // layouts: bshd = [B, S, H, D] (strided views allowed),
    //          else  = [B, H, S, D] (must be row-contiguous per head)
    const int b_ax = 0, s_ax = bshd ? 1 : 2, h_ax = bshd ? 2 : 1, d_ax = 3;
    const int B = (int)q.size(b_ax), S = (int)q.size(s_ax),
              H = (int)q.size(h_ax), D = (int)q.size(d_ax);
    TORCH_CHECK(D == 64 || D == 128, "attn_fwd: D must be 64 or 128");
    auto fix = [&](at::Tensor t) {
        if (t.stride(d_ax) != 1 || (t.stride(s_ax) % 8) != 0 ||
            (t.stride(h_ax) % 8) != 0)
            t = t.contiguous();
        return t;
    };
    auto qc = fix(q);
    auto kc = fix(k);
    auto vc = fix(v);
    const int Sk = (int)kc.size(s_ax);
    TORCH_CHECK((int)vc.size(s_ax) == Sk && (int)kc.size(h_ax) == H,
                "attn: k/v shape mismatch");
    if (km != nullptr) {
        const long n_tiles = (Sk + 63) / 64;
        TORCH_CHECK(km->words.device() == qc.device() &&
                        km->live.device() == qc.device() &&
                        km->nlive.device() == qc.device(),
                    "attn_fwd: key mask must be on q's device");
        TORCH_CHECK(km->words.scalar_type() == at::kLong &&
                        km->live.scalar_type() == at::kInt &&
                        km->nlive.scalar_type() == at::kInt,
                    "attn_fwd: key mask needs int64 words, int32 live/nlive");
        TORCH_CHECK(km->words.dim() == 2 && km->live.dim() == 2 &&
                        km->nlive.dim() == 1 && km->words.size(0) == B &&
                        km->live.size(0) == B && km->nlive.size(0) == B,
                    "attn_fwd: key mask batch must equal q's batch (", B, ")");
        TORCH_CHECK(km->words.size(1) == n_tiles &&
                        km->live.size(1) == n_tiles,
                    "attn_fwd: key mask was packed for another Sk (", Sk,
                    " keys need ", n_tiles, " tiles, got ",
                    km->words.size(1), ")");
        TORCH_CHECK(km->words.is_contiguous() && km->live.is_contiguous() &&
                        km->nlive.is_contiguous(),
                    "attn_fwd: key mask tensors must be contiguous");
    }
    const bool do_split = split > 0 && split < S && bshd;
    at::Tensor out = bshd
        ? at::empty({B, do_split ? (int)split : S, H, D}, qc.options())
        : at::empty({B, H, S, D}, qc.options());
    at::Tensor out2;
    if (do_split) out2 = at::empty({B, S - (int)split, H, D}, qc.options());
    static const bool use_v3 = []() {
        const char* e = getenv("PA_ATTN_V3");
        return e && e[0] == '1';
    }();
    // the previous-generation debug kernel has no fp16 instantiation; its
    // bf16 conversions must never see fp16 bits
    TORCH_CHECK(!use_v3 || qc.scalar_type() == at::kBFloat16,
                "attn_fwd: PA_ATTN_V3=1 selects the bf16-only debug kernel; "
                "got ", qc.scalar_type(), " — unset PA_ATTN_V3 for fp16");
    TORCH_CHECK(!use_v3 || km == nullptr,
                "attn_fwd: PA_ATTN_V3=1 selects the debug kernel, which has "
                "no key mask — unset PA_ATTN_V3 for masked attention");
    TORCH_CHECK(!use_v3 || !do_split, "split output needs the v4 kernel");
    const long BH = (long)B * H;
    const unsigned nq = (unsigned)((S + 255) / 256);
    // 1-D XCD-affine grid (v4 only): same-(b,h) q-tiles share an XCD's L2
    const bool xcd_grid = !use_v3 && BH % 8 == 0;
    const dim3 grid = xcd_grid ? dim3((unsigned)(nq * BH), 1)
                               : dim3(nq, (unsigned)BH);
    const AttnArgs a{
        qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
        S, Sk, (float)scale, H,
        qc.stride(b_ax), qc.stride(h_ax), (int)qc.stride(s_ax),
        kc.stride(b_ax), kc.stride(h_ax), (int)kc.stride(s_ax),
        vc.stride(b_ax), vc.stride(h_ax), (int)vc.stride(s_ax),
        out.stride(b_ax), out.stride(h_ax), (int)out.stride(s_ax),
        xcd_grid ? 1 : 0,
        do_split ? out2.data_ptr() : nullptr, do_split ? (int)split : S,
        do_split ? out2.stride(0) : 0, do_split ? out2.stride(2) : 0,
        do_split ? (int)out2.stride(1) : 0,
        km ? (const unsigned long long*)km->words.data_ptr() : nullptr,
        km ? km->live.data_ptr<int>() : nullptr,
        km ? km->nlive.data_ptr<int>() : nullptr};
    const at::ScalarType st = qc.scalar_type();
    if (use_v3) {
        if (D == 128) launch_attn_v3<128>(grid, a);
        else launch_attn_v3<64>(grid, a);
    } else if (km != nullptr) {
        if (D == 128) launch_attn_v4<128, true>(st, grid, a);
        else launch_attn_v4<64, true>(st, grid, a);
    } else {
        if (D == 128) launch_attn_v4<128, false>(st, grid, a);
        else launch_attn_v4<64, false>(st, grid, a);
    }
    if (do_split) return {out, out2};
    return {out};
}

at::Tensor attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v, double scale) {
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/false, -1, nullptr)[0];
}

at::Tensor attn_fwd_bshd(at::Tensor q, at::Tensor k, at::Tensor v, double scale) {
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, -1, nullptr)[0];
}

std::vector<at::Tensor> attn_fwd_bshd_split(at::Tensor q, at::Tensor k,
                                            at::Tensor v, double scale,
                                            long split) {
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, split, nullptr);
}

at::Tensor attn_fwd_masked(at::Tensor q, at::Tensor k, at::Tensor v,
                           double scale, at::Tensor words, at::Tensor live,
                           at::Tensor nlive) {
    const AttnKeyMask km{words, live, nlive};
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/false, -1, &km)[0];
}

at::Tensor attn_fwd_bshd_masked(at::Tensor q, at::Tensor k, at::Tensor v,
                                double scale, at::Tensor words,
                                at::Tensor live, at::Tensor nlive) {
    const AttnKeyMask km{words, live, nlive};
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, -1, &km)[0];
}

std::vector<at::Tensor> attn_fwd_bshd_split_masked(
    at::Tensor q, at::Tensor k, at::Tensor v, double scale, long split,
    at::Tensor words, at::Tensor live, at::Tensor nlive) {
    const AttnKeyMask km{words, live, nlive};
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, split, &km);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("rms_norm", &rms_norm, "RMSNorm (gfx950)",
          py::arg("x"), py::arg("weight") = py::none(), py::arg("eps") = 1e-6);
    m.def("layer_norm_mod", &layer_norm_mod, "AdaLN-modulated LayerNorm (gfx950)");
    m.def("layer_norm_mod_fp8", &layer_norm_mod_fp8,
          "AdaLN LayerNorm with fused e4m3fn quant + delayed scaling (gfx950)");
    m.def("gate_residual", &gate_residual, "Gated residual add (gfx950)");
    m.def("group_norm_silu", &group_norm_silu, "GroupNorm+SiLU (gfx950)",
          py::arg("x"), py::arg("groups"), py::arg("weight") = py::none(),
          py::arg("bias") = py::none(), py::arg("eps") = 1e-6);
    m.def("rope_apply", &rope_apply, "RoPE apply (gfx950)");
    m.def("timestep_embedding", &timestep_embedding, "Sinusoidal timestep embedding");
    m.def("attn_fwd", &attn_fwd,
          "Fused flash attention fwd, bf16/fp16 MFMA (gfx950)");
    m.def("attn_fwd_bshd", &attn_fwd_bshd,
          "Fused flash attention fwd on [B,S,H,D] strided views (gfx950)");
    m.def("attn_fwd_bshd_split", &attn_fwd_bshd_split,
          "Attention with per-stream split outputs [B,:split]/[B,split:]");
    m.def("pack_key_mask", &pack_key_mask,
          "[B,Sk] bool/int key mask -> (words, live tile list, nlive)");
    m.def("attn_fwd_masked", &attn_fwd_masked,
          "attn_fwd with a packed key-padding mask (dead tiles skipped)");
    m.def("attn_fwd_bshd_masked", &attn_fwd_bshd_masked,
          "attn_fwd_bshd with a packed key-padding mask");
    m.def("attn_fwd_bshd_split_masked", &attn_fwd_bshd_split_masked,
          "attn_fwd_bshd_split with a packed key-padding mask");
    m.def("gelu_tanh", &gelu_tanh, "Vectorized tanh-GELU (gfx950)");
    m.def("gelu_fp8", &gelu_fp8,
          "tanh-GELU with fused e4m3fn quant + delayed scaling (gfx950)");
    m.def("quant_fp8", &quant_fp8,
          "Fused bf16->e4m3fn quant with running amax (gfx950)");
    m.def("timestep_embed_mlp", &timestep_embed_mlp,
          "Fused sinusoidal embed + Linear + SiLU (gfx950)");
    m.def("pack_joint_qkv", &pack_joint_qkv,
          "Fused dual-stream qkv pack + qk-norm + RoPE (gfx950)");
    m.def("qk_norm_rope_", &qk_norm_rope_,
          "In-place fused qk RMSNorm + RoPE on [B,S,H,D] views (gfx950)");
}
