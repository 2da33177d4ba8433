// qk_norm_rope_ / pack_joint_qkv A/B (gfx950): the shipped generic kernels
// (one pair per lane, 4 rows per wave) against the token-major kernels (8
// elements per lane, whole tokens per wave) at several depths CH and with
// DPP or __shfl_xor exchanges, and against a 16-byte-per-lane passthrough
// over the same bytes, which is the ceiling of the access pattern. The
// kernels are the text the extension compiles (ops/hip/qk_pack_kernels.h).
//
// Every token-major variant first passes a bitwise gate against the generic
// kernel: same input, whole buffers compared, at small shapes where waves
// straddle tokens and end in partial rows, and at the flagship shape.
// Timing: variants interleaved in one process, best..worst round reported.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 qknr_ab.hip -o qknr
// Run:   ./qknr [rounds]     gate + timing tables
//        ./qknr pmc          a few calls of generic, shipped and passthrough
//                            only (for rocprofv3 --pmc, no tracing beside it)
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <functional>
#include <algorithm>

#define PA_DEV __device__ __forceinline__
using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(8))) short short8;
template <typename E> struct Elem16;
template <> struct Elem16<bf16> {
    static PA_DEV float ld(unsigned short u) {
        return __bfloat162float(__ushort_as_bfloat16(u));
    }
    static PA_DEV unsigned short st(float f) {
        return __bfloat16_as_ushort(__float2bfloat16(f));
    }
};
template <> struct Elem16<_Float16> {
    static PA_DEV float ld(unsigned short u) {
        return (float)__builtin_bit_cast(_Float16, u);
    }
    static PA_DEV unsigned short st(float f) {
        return __builtin_bit_cast(unsigned short, (_Float16)f);
    }
};
PA_DEV float wave_reduce_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
#include "../comfyui_parallelanything_amd/ops/hip/qk_pack_kernels.h"

#define HIP_CHECK(x) do { hipError_t e = (x); if (e) { \
    printf("HIP error %d (%s) at line %d\n", e, hipGetErrorString(e), \
           __LINE__); exit(1); } } while (0)

// ---- data ------------------------------------------------------------------
__device__ __forceinline__ unsigned mix(unsigned long i, unsigned seed) {
    unsigned x = (unsigned)i * 2654435761u ^ (unsigned)(i >> 32) ^ seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu;
    return x ^ (x >> 16);
}
// uniform [-1, 1) values; every 7th run of `row` elements scaled by 30 and
// every 11th all zero, so the rows are not of one scale
template <typename E>
__global__ void fill_kernel(E* p, long n, int row, unsigned seed) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        const long r = i / row;
        const float sc = r % 11 == 5 ? 0.f : (r % 7 == 3 ? 30.f : 1.f);
        const float f = ((mix(i, seed) >> 8) / 8388608.0f - 1.f) * sc;
        p[i] = (E)f;
    }
}
__global__ void fill_cs_kernel(float* cs, long pairs) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < pairs;
         i += (long)gridDim.x * blockDim.x) {
        const float a = (mix(i, 99u) >> 8) / 8388608.0f * 3.14159265f;
        cs[2 * i] = cosf(a);
        cs[2 * i + 1] = sinf(a);
    }
}
__global__ void diff_kernel(const unsigned* a, const unsigned* b, long n,
                            unsigned long long* count) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x)
        if (a[i] != b[i]) atomicAdd(count, 1ull);
}

// 16 bytes per lane, read-modify-write (NW = 2: q and k in place) or
// read 3 / write 3 elsewhere (NW = 3: the pack), same token walk as the
// token-major kernels at CH = 3 and no arithmetic but a sign flip (a plain
// store of the loaded value would be dropped).
template <int NW>
__global__ void __launch_bounds__(256)
passthrough_kernel(short8* __restrict__ src, short8* __restrict__ dst,
                   long tok_stride8, long slot8, int hd8, unsigned nchunk,
                   unsigned n_work) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= n_work) return;
    const unsigned tok = wave / nchunk, chunk = wave % nchunk;
    short8* s = src + tok * tok_stride8;
    short8* d = dst ? dst + (long)tok * hd8 : nullptr;
    short8 v[3][NW];
    int off[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int o = (chunk * 3 + i) * 64 + lane;
        off[i] = o < hd8 ? o : -1;
#pragma unroll
        for (int w = 0; w < NW; ++w) v[i][w] = s[w * slot8 + (o < hd8 ? o : 0)];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (off[i] < 0) continue;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            short8 x = v[i][w];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] ^= (short)0x8000;
            if (d) d[(long)w * n_work / nchunk * hd8 + off[i]] = x;
            else s[w * slot8 + off[i]] = x;
        }
    }
}

struct Shape { int B, T, S, H, D; const char* name; };  // T: txt tokens (pack)

template <typename E>
struct Probe {
    Shape sh;
    long n, tok_stride, slot;   // qkv buffer [B, S, 3, H, D]
    E *init, *work, *ref, *w;
    E *o_ref, *o_got;           // pack outputs, 3 x [B, S, H, D] each
    float* cs;
    unsigned long long* cnt;
    long out_n;

    explicit Probe(Shape s, bool with_pack) : sh(s) {
        slot = (long)s.H * s.D;
        tok_stride = 3 * slot;
        n = (long)s.B * s.S * tok_stride;
        out_n = 3 * (long)s.B * s.S * slot;
        HIP_CHECK(hipMalloc(&init, n * 2));
        HIP_CHECK(hipMalloc(&work, n * 2));
        HIP_CHECK(hipMalloc(&ref, n * 2));
        HIP_CHECK(hipMalloc(&w, 4 * 128 * 2));
        HIP_CHECK(hipMalloc(&cs, (long)s.S * s.D * 4));
        HIP_CHECK(hipMalloc(&cnt, 8));
        o_ref = o_got = nullptr;
        if (with_pack) {
            HIP_CHECK(hipMalloc(&o_ref, out_n * 2));
            HIP_CHECK(hipMalloc(&o_got, out_n * 2));
        }
        hipLaunchKernelGGL(fill_kernel<E>, dim3(2048), dim3(256), 0, 0, init,
                           n, s.D, 7u);
        hipLaunchKernelGGL(fill_kernel<E>, dim3(2), dim3(256), 0, 0, w,
                           4L * 128, 1 << 20, 13u);
        hipLaunchKernelGGL(fill_cs_kernel, dim3(256), dim3(256), 0, 0, cs,
                           (long)s.S * s.D / 2);
        HIP_CHECK(hipDeviceSynchronize());
    }
    ~Probe() {
        (void)hipFree(init); (void)hipFree(work); (void)hipFree(ref);
        (void)hipFree(w); (void)hipFree(cs); (void)hipFree(cnt);
        if (o_ref) { (void)hipFree(o_ref); (void)hipFree(o_got); }
    }
    void reset() { HIP_CHECK(hipMemcpy(work, init, n * 2, hipMemcpyDeviceToDevice)); }
    unsigned long long diff(const void* a, const void* b, long elems) {
        HIP_CHECK(hipMemset(cnt, 0, 8));
        hipLaunchKernelGGL(diff_kernel, dim3(2048), dim3(256), 0, 0,
                           (const unsigned*)a, (const unsigned*)b, elems / 2,
                           cnt);
        unsigned long long h;
        HIP_CHECK(hipMemcpy(&h, cnt, 8, hipMemcpyDeviceToHost));
        return h;
    }

    // ---- qk_norm_rope_ on q = slot 0, k = slot 1 of `work` -----------------
    void qk_generic() {
        const long rows = (long)sh.B * sh.S * sh.H;
        const long blocks = (((rows + 3) / 4) * 64 + 255) / 256;
        const long bs = (long)sh.S * tok_stride;
        hipLaunchKernelGGL(qk_norm_rope_kernel<E>, dim3((unsigned)blocks),
                           dim3(256), 0, 0, work, work + slot, w, w + 128, cs,
                           sh.S, sh.H, sh.D, bs, (long)sh.D, tok_stride, bs,
                           (long)sh.D, tok_stride, rows, 1e-6f);
    }
    template <int DT, int CH, bool kDpp>
    void qk_tok_d() {
        const int HD = sh.H * sh.D;
        const unsigned nchunk = (HD + CH * 512 - 1) / (CH * 512);
        const unsigned nw = (unsigned)sh.B * sh.S * nchunk;
        const long bs = (long)sh.S * tok_stride;
        hipLaunchKernelGGL((qk_norm_rope_tok_kernel<E, DT, CH, kDpp>),
                           dim3((nw + 3) / 4), dim3(256), 0, 0, work,
                           work + slot, w, w + 128, cs, (unsigned)sh.S, HD,
                           sh.D, bs, tok_stride, bs, tok_stride, nchunk, nw,
                           1e-6f);
    }
    template <int CH, bool kDpp>
    void qk_tok() {
        if (sh.D == 128) qk_tok_d<128, CH, kDpp>();
        else qk_tok_d<64, CH, kDpp>();
    }
    void qk_pass() {
        const int hd8 = sh.H * sh.D / 8;
        const unsigned nchunk = (hd8 + 3 * 64 - 1) / (3 * 64);
        const unsigned nw = (unsigned)sh.B * sh.S * nchunk;
        hipLaunchKernelGGL(passthrough_kernel<2>, dim3((nw + 3) / 4),
                           dim3(256), 0, 0, (short8*)work, (short8*)nullptr,
                           tok_stride / 8, slot / 8, hd8, nchunk, nw);
    }

    // ---- pack_joint_qkv: tokens [0, T) of `init` are txt, the rest img -----
    void pack_generic(E* out) {
        const long rows = (long)sh.B * sh.S * sh.H;
        const long blocks = (((rows + 3) / 4) * 64 + 255) / 256;
        const long bs = (long)sh.S * tok_stride, on = out_n / 3;
        hipLaunchKernelGGL(pack_joint_qkv_kernel<E>, dim3((unsigned)blocks),
                           dim3(256), 0, 0, init, init + sh.T * tok_stride, w,
                           w + 128, w + 256, w + 384, cs, out, out + on,
                           out + 2 * on, sh.T, sh.S - sh.T, sh.H, sh.D, bs,
                           tok_stride, slot, (long)sh.D, bs, tok_stride, slot,
                           (long)sh.D, rows, 1e-6f);
    }
    template <int DT, int CH, bool kDpp>
    void pack_tok_d(E* out) {
        const int HD = sh.H * sh.D;
        const unsigned nchunk = (HD + CH * 512 - 1) / (CH * 512);
        const unsigned nw = (unsigned)sh.B * sh.S * nchunk;
        const long bs = (long)sh.S * tok_stride, on = out_n / 3;
        hipLaunchKernelGGL((pack_joint_qkv_tok_kernel<E, DT, CH, kDpp>),
                           dim3((nw + 3) / 4), dim3(256), 0, 0, init,
                           init + sh.T * tok_stride, w, w + 128, w + 256,
                           w + 384, cs, out, out + on, out + 2 * on,
                           (unsigned)sh.T, (unsigned)sh.S, HD, sh.D, bs,
                           tok_stride, slot, bs, tok_stride, slot, nchunk, nw,
                           1e-6f);
    }
    template <int CH, bool kDpp>
    void pack_tok(E* out) {
        if (sh.D == 128) pack_tok_d<128, CH, kDpp>(out);
        else pack_tok_d<64, CH, kDpp>(out);
    }
    void pack_pass(E* out) {
        const int hd8 = sh.H * sh.D / 8;
        const unsigned nchunk = (hd8 + 3 * 64 - 1) / (3 * 64);
        const unsigned nw = (unsigned)sh.B * sh.S * nchunk;
        hipLaunchKernelGGL(passthrough_kernel<3>, dim3((nw + 3) / 4),
                           dim3(256), 0, 0, (short8*)init, (short8*)out,
                           tok_stride / 8, slot / 8, hd8, nchunk, nw);
    }

    // every token-major variant against the generic kernel, bit for bit
    bool gate(bool with_pack) {
        bool ok = true;
        reset(); qk_generic();
        HIP_CHECK(hipMemcpy(ref, work, n * 2, hipMemcpyDeviceToDevice));
        std::vector<std::pair<const char*, std::function<void()>>> qv = {
            {"CH2 dpp", [&] { qk_tok<2, true>(); }},
            {"CH3 dpp", [&] { qk_tok<3, true>(); }},
            {"CH6 dpp", [&] { qk_tok<6, true>(); }},
            {"CH3 shfl", [&] { qk_tok<3, false>(); }},
        };
        for (auto& v : qv) {
            reset(); v.second();
            HIP_CHECK(hipGetLastError());
            const auto d = diff(ref, work, n);
            if (d) { ok = false; printf("  qk   %-9s %s: %llu words differ\n", v.first, sh.name, d); }
        }
        if (with_pack) {
            pack_generic(o_ref);
            std::vector<std::pair<const char*, std::function<void()>>> pv = {
                {"CH2 dpp", [&] { pack_tok<2, true>(o_got); }},
                {"CH3 dpp", [&] { pack_tok<3, true>(o_got); }},
                {"CH6 dpp", [&] { pack_tok<6, true>(o_got); }},
                {"CH3 shfl", [&] { pack_tok<3, false>(o_got); }},
            };
            for (auto& v : pv) {
                HIP_CHECK(hipMemset(o_got, 0xff, out_n * 2));
                v.second();
                HIP_CHECK(hipGetLastError());
                const auto d = diff(o_ref, o_got, out_n);
                if (d) { ok = false; printf("  pack %-9s %s: %llu words differ\n", v.first, sh.name, d); }
            }
        }
        HIP_CHECK(hipDeviceSynchronize());
        printf("gate %-28s %s\n", sh.name, ok ? "bit-equal" : "MISMATCH");
        return ok;
    }
};

static void time_table(const char* title, double gb, int rounds,
    std::vector<std::pair<const char*, std::function<void()>>>& vs) {
    const size_t nv = vs.size();
    std::vector<double> best(nv, 1e30), worst(nv, 0.);
    for (auto& v : vs) v.second();
    HIP_CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    for (int r = 0; r < rounds; ++r)
        for (size_t i = 0; i < nv; ++i) {
            HIP_CHECK(hipEventRecord(e0));
            for (int it = 0; it < 3; ++it) vs[i].second();
            HIP_CHECK(hipEventRecord(e1));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            best[i] = std::min(best[i], ms / 3.0);
            worst[i] = std::max(worst[i], ms / 3.0);
        }
    printf("%s (%.3f GB moved, %d rounds of 3 calls, us best..worst, TB/s at best)\n",
           title, gb, rounds);
    for (size_t i = 0; i < nv; ++i)
        printf("  %-22s %8.1f .. %8.1f us   %5.2f TB/s\n", vs[i].first,
               best[i] * 1e3, worst[i] * 1e3, gb / best[i]);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
}

template <typename E>
static bool gates(const char* tag) {
    const Shape small[] = {
        {2, 3, 8, 3, 128, "B2 T3+5 H3 D128"}, {2, 3, 8, 3, 64, "B2 T3+5 H3 D64"},
        {2, 0, 5, 3, 128, "B2 T0+5 H3 D128"}, {1, 0, 1, 1, 128, "B1 S1 H1 D128"},
        {1, 0, 1, 1, 64, "B1 S1 H1 D64"},
        {2, 64, 134, 24, 128, "B2 T64+70 H24 D128"},
        {2, 64, 134, 24, 64, "B2 T64+70 H24 D64"},
        {2, 5, 9, 38, 64, "B2 T5+4 H38 D64"}, {1, 2, 7, 30, 128, "B1 T2+5 H30 D128"},
    };
    bool ok = true;
    printf("[%s]\n", tag);
    for (const Shape& s : small) {
        Probe<E> p(s, true);
        ok = p.gate(true) && ok;
    }
    return ok;
}

int main(int argc, char** argv) {
    const bool pmc = argc > 1 && !strcmp(argv[1], "pmc");
    const int rounds = (!pmc && argc > 1) ? atoi(argv[1]) : 10;
    // flux single block: q/k views of [8, 4608, 3, 24, 128]; the double
    // block's pack reads 512 txt + 4096 img tokens of the same layout
    const Shape flux = {8, 512, 4608, 24, 128, "flux B8 S4608 H24 D128"};
    if (pmc) {
        Probe<bf16> p(flux, true);
        for (int i = 0; i < 3; ++i) {
            p.qk_generic(); p.qk_tok<2, true>(); p.qk_pass();
            p.pack_generic(p.o_ref); p.pack_tok<2, true>(p.o_got);
            p.pack_pass(p.o_got);
        }
        HIP_CHECK(hipDeviceSynchronize());
        return 0;
    }
    bool ok = gates<bf16>("bf16");
    ok = gates<_Float16>("fp16") && ok;
    Probe<bf16> p(flux, true);
    ok = p.gate(true) && ok;
    if (!ok) { printf("gate FAILED: no timing\n"); return 1; }

    const double rows = (double)flux.B * flux.S * flux.H;
    std::vector<std::pair<const char*, std::function<void()>>> qv = {
        {"generic (parent)", [&] { p.qk_generic(); }},
        {"tok CH2 dpp", [&] { p.qk_tok<2, true>(); }},
        {"tok CH3 dpp", [&] { p.qk_tok<3, true>(); }},
        {"tok CH6 dpp", [&] { p.qk_tok<6, true>(); }},
        {"tok CH2 shfl", [&] { p.qk_tok<2, false>(); }},
        {"tok CH3 shfl", [&] { p.qk_tok<3, false>(); }},
        {"passthrough 16B rmw", [&] { p.qk_pass(); }},
    };
    p.reset();
    time_table("qk_norm_rope_ flux", rows * flux.D * 2 * 2 * 2 / 1e9, rounds, qv);
    std::vector<std::pair<const char*, std::function<void()>>> pv = {
        {"generic (parent)", [&] { p.pack_generic(p.o_ref); }},
        {"tok CH2 dpp", [&] { p.pack_tok<2, true>(p.o_got); }},
        {"tok CH3 dpp", [&] { p.pack_tok<3, true>(p.o_got); }},
        {"tok CH6 dpp", [&] { p.pack_tok<6, true>(p.o_got); }},
        {"tok CH2 shfl", [&] { p.pack_tok<2, false>(p.o_got); }},
        {"tok CH3 shfl", [&] { p.pack_tok<3, false>(p.o_got); }},
        {"passthrough 16B copy", [&] { p.pack_pass(p.o_got); }},
    };
    time_table("pack_joint_qkv flux", rows * flux.D * 2 * 3 * 2 / 1e9, rounds, pv);
    return 0;
}
