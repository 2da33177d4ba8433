// layer_norm_mod_vec_kernel A/B (gfx950): the shipped kernel (two passes
// over the row, two block reductions, four barriers) against a form that
// keeps each thread's vectors in registers between the statistics and the
// modulate pass and exchanges both sums in one LDS round (one barrier), with
// and without the scale/shift loads issued before the reduction; and
// against a 16-byte-per-lane copy of the same bytes, the ceiling.
//
// The candidates keep the thread-to-element assignment, the per-thread add
// order, the wave butterfly and the scratch[0..3] add order, and pass a
// bitwise gate against the shipped kernel before anything is timed.
// The "shipped" text below is a copy of ops/hip/norm.h (kernel and helpers).
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 lnmod_ab.hip -o lnmod
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <functional>
#include <algorithm>

#define PA_DEV __device__ __forceinline__
using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(2))) float f32x2;
static constexpr int WAVE = 64;
template <typename E> struct Elem16;
template <> struct Elem16<bf16> {
    static PA_DEV float ld(unsigned short u) {
        return __bfloat162float(__ushort_as_bfloat16(u));
    }
    static PA_DEV unsigned short st(float f) {
        return __bfloat16_as_ushort(__float2bfloat16(f));
    }
};
#define HIP_CHECK(x) do { hipError_t e = (x); if (e) { \
    printf("HIP error %d (%s) at line %d\n", e, hipGetErrorString(e), \
           __LINE__); exit(1); } } while (0)

// ---- shipped (ops/hip/common.h, norm.h) --------------------------------------
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
    __syncthreads();
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) total += scratch[i];
    return total;
}
template <typename EL>
PA_DEV f32x2 ln_row_sums(const short8* xr, int D) {
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
    float var = block_reduce_sum<256>(s[1], scratch) / (float)D - mean * mean;
    rstd = rsqrtf(fmaxf(var, 0.f) + eps);
}
template <typename EL>
PA_DEV float ln_modulate(short x, short scale, short shift, float mean,
                         float rstd) {
    float f = (EL::ld((unsigned short)x) - mean) * rstd;
    return f * (1.f + EL::ld((unsigned short)scale)) +
           EL::ld((unsigned short)shift);
}
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

// ---- candidate: rows of up to NV * 256 vectors held in registers --------------
template <typename E, int NV, bool kEarly>
__global__ void __launch_bounds__(256)
lnmod_reg_kernel(const E* __restrict__ x, const E* __restrict__ scale,
                 const E* __restrict__ shift, E* __restrict__ out, int S,
                 int D, long sc_rs, long sh_rs, float eps) {
    using EL = Elem16<E>;
    const long row = blockIdx.x;
    const long b = row / S;
    const short8* xr = reinterpret_cast<const short8*>(x + row * (long)D);
    const short8* sc = reinterpret_cast<const short8*>(scale + b * sc_rs);
    const short8* sh = reinterpret_cast<const short8*>(shift + b * sh_rs);
    short8* yr = reinterpret_cast<short8*>(out + row * (long)D);
    const int DV = D / 8;
    __shared__ float scratch[8];

    short8 v[NV], a[NV], c[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < DV) {
            v[k] = xr[i];
            if (kEarly) { a[k] = sc[i]; c[k] = sh[i]; }
        }
    }
    f32x2 s = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        if ((int)threadIdx.x + k * 256 < DV) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float f = EL::ld((unsigned short)v[k][j]);
                s += f32x2{f, f * f};
            }
        }
    }
    const float w0 = wave_reduce_sum(s[0]), w1 = wave_reduce_sum(s[1]);
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    if (lane == 0) { scratch[wid] = w0; scratch[4 + wid] = w1; }
    __syncthreads();
    float t0 = 0.f, t1 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) t0 += scratch[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) t1 += scratch[4 + i];
    const float mean = t0 / (float)D;
    float var = t1 / (float)D - mean * mean;
    const float rstd = rsqrtf(fmaxf(var, 0.f) + eps);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < DV) {
            if (!kEarly) { a[k] = sc[i]; c[k] = sh[i]; }
            short8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                o[j] = (short)EL::st(
                    ln_modulate<EL>(v[k][j], a[k][j], c[k][j], mean, rstd));
            yr[i] = o;
        }
    }
}

__global__ void copy_kernel(const short8* __restrict__ x,
                            short8* __restrict__ out, int DV) {
    const short8* xr = x + (long)blockIdx.x * DV;
    short8* yr = out + (long)blockIdx.x * DV;
    for (int i = threadIdx.x; i < DV; i += blockDim.x) {
        short8 v = xr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] ^= (short)0x8000;
        yr[i] = v;
    }
}

__device__ __forceinline__ unsigned mix(unsigned long i, unsigned seed) {
    unsigned x = (unsigned)i * 2654435761u ^ (unsigned)(i >> 32) ^ seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu;
    return x ^ (x >> 16);
}
// uniform [-1, 1) + a row mean; every 7th row scaled by 30, every 11th zero
__global__ void fill_kernel(bf16* p, long n, int row, unsigned seed,
                            float amp) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        const long r = i / row;
        const float sc = r % 11 == 5 ? 0.f : (r % 7 == 3 ? 30.f : 1.f);
        const float m = (float)(r % 5) - 2.f;
        p[i] = (bf16)((((mix(i, seed) >> 8) / 8388608.0f - 1.f) + m) * sc * amp);
    }
}
__global__ void diff_kernel(const unsigned* a, const unsigned* b, long n,
                            unsigned long long* count) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x)
        if (a[i] != b[i]) atomicAdd(count, 1ull);
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 10;
    struct Shape { int B, S, D; };
    // gate-only shapes first (D / 8 below, at and above 256 vectors, not a
    // multiple of 256), then the three timed ones
    const Shape shapes[] = {{2, 3, 72}, {2, 5, 2048}, {3, 7, 2056}, {2, 3, 4096},
                            {8, 4608, 3072}, {8, 4096, 3072}, {8, 512, 3072}};
    const int BANK = 5;   // scale/shift are column slices of [B, 5 D]
    unsigned long long* cnt;
    HIP_CHECK(hipMalloc(&cnt, 8));
    for (const Shape& sh : shapes) {
        const long n = (long)sh.B * sh.S * sh.D;
        const long rs = (long)BANK * sh.D;
        bf16 *x, *bank, *ref, *got;
        HIP_CHECK(hipMalloc(&x, n * 2));
        HIP_CHECK(hipMalloc(&ref, n * 2));
        HIP_CHECK(hipMalloc(&got, n * 2));
        HIP_CHECK(hipMalloc(&bank, sh.B * rs * 2));
        hipLaunchKernelGGL(fill_kernel, dim3(2048), dim3(256), 0, 0, x, n,
                           sh.D, 3u, 1.f);
        hipLaunchKernelGGL(fill_kernel, dim3(64), dim3(256), 0, 0, bank,
                           sh.B * rs, 1 << 30, 5u, 0.25f);
        const bf16* sc = bank + sh.D;
        const bf16* sf = bank + 3 * sh.D;
        const dim3 grid((unsigned)(sh.B * sh.S));
        auto shipped = [&](bf16* o) {
            hipLaunchKernelGGL(layer_norm_mod_vec_kernel<bf16>, grid,
                               dim3(256), 0, 0, x, sc, sf, o, sh.S, sh.D, rs,
                               rs, 1e-6f);
        };
        auto reg_late = [&](bf16* o) {
            hipLaunchKernelGGL((lnmod_reg_kernel<bf16, 2, false>), grid,
                               dim3(256), 0, 0, x, sc, sf, o, sh.S, sh.D, rs,
                               rs, 1e-6f);
        };
        auto reg_early = [&](bf16* o) {
            hipLaunchKernelGGL((lnmod_reg_kernel<bf16, 2, true>), grid,
                               dim3(256), 0, 0, x, sc, sf, o, sh.S, sh.D, rs,
                               rs, 1e-6f);
        };
        auto copy = [&](bf16* o) {
            hipLaunchKernelGGL(copy_kernel, grid, dim3(256), 0, 0,
                               (const short8*)x, (short8*)o, sh.D / 8);
        };
        shipped(ref);
        bool ok = true;
        for (int v = 0; v < 2; ++v) {
            HIP_CHECK(hipMemset(got, 0xff, n * 2));
            if (v == 0) reg_late(got); else reg_early(got);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemset(cnt, 0, 8));
            hipLaunchKernelGGL(diff_kernel, dim3(2048), dim3(256), 0, 0,
                               (const unsigned*)ref, (const unsigned*)got,
                               n / 2, cnt);
            unsigned long long h;
            HIP_CHECK(hipMemcpy(&h, cnt, 8, hipMemcpyDeviceToHost));
            if (h) { ok = false; printf("  variant %d: %llu words differ\n", v, h); }
        }
        printf("gate [%d, %d, %d] %s\n", sh.B, sh.S, sh.D,
               ok ? "bit-equal" : "MISMATCH");
        if (!ok) return 1;
        if (sh.B * sh.S >= 4096) {
            std::vector<std::pair<const char*, std::function<void()>>> vs = {
                {"shipped", [&] { shipped(got); }},
                {"registers", [&] { reg_late(got); }},
                {"registers, early mod", [&] { reg_early(got); }},
                {"16B copy", [&] { copy(got); }},
            };
            std::vector<double> best(vs.size(), 1e30), worst(vs.size(), 0.);
            for (auto& v : vs) v.second();
            HIP_CHECK(hipDeviceSynchronize());
            hipEvent_t e0, e1;
            HIP_CHECK(hipEventCreate(&e0));
            HIP_CHECK(hipEventCreate(&e1));
            for (int r = 0; r < rounds; ++r)
                for (size_t i = 0; i < vs.size(); ++i) {
                    HIP_CHECK(hipEventRecord(e0));
                    for (int it = 0; it < 5; ++it) vs[i].second();
                    HIP_CHECK(hipEventRecord(e1));
                    HIP_CHECK(hipEventSynchronize(e1));
                    float ms;
                    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
                    best[i] = std::min(best[i], ms / 5.0);
                    worst[i] = std::max(worst[i], ms / 5.0);
                }
            const double gb = n * 2.0 * 2 / 1e9;
            printf("[%d, %d, %d] %.3f GB moved, %d rounds of 5 calls\n", sh.B,
                   sh.S, sh.D, gb, rounds);
            for (size_t i = 0; i < vs.size(); ++i)
                printf("  %-22s %7.1f .. %7.1f us   %5.2f TB/s\n", vs[i].first,
                       best[i] * 1e3, worst[i] * 1e3, gb / best[i]);
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
        }
        (void)hipFree(x); (void)hipFree(ref); (void)hipFree(got);
        (void)hipFree(bank);
    }
    return 0;
}
