// v6 softmax-VALU A/B harness (gfx950): work the result never needs.
//
// The shipped attention (attn_fwd_v4_kernel: v5a one-barrier pipeline at
// D=128, two-barrier loop at D=64) spends ~100 of its ~330 per-tile issue
// slots on a per-key `key < Sk` test that is true on every tile but a last
// partial one, and exchanges the row max / row sum between half-waves with
// two ds_bpermute round trips (each followed by a full lgkmcnt(0) wait).
// This probe times the removal of both, plus the scalar-vs-packed alpha
// rescale, against the shipped code in one process.
//
// OPT bits (template parameter of attn_v6_kernel):
//   1  FULL   no per-key work on a full tile. The -3e30 substitution runs
//             in place on the scores under a block-uniform scalar branch
//             (`if (!full)`), ahead of ONE softmax body without any key
//             index / compare / select
//   2  SWAP   half-wave max/sum exchange by v_permlane32_swap, not LDS
//   4  SMUL   alpha rescale kept as 64 scalar v_mul_f32 (no v_pk_mul_f32)
//   16 TWO    (with FULL) the branch picks between two complete softmax
//             bodies, a FULL one and the shipped one, instead
//   8  PEEL   (with TWO) the KV loop runs nt-1 branch-free full tiles and
//             only the peeled last tile tests; unmasked only — a masked
//             word can be partial anywhere, so MASKED keeps the branch
//
// Variants, interleaved within the probe (same process, same buffers):
//   v0 = 0 shipped   v1 = {1}   v2 = {1+2}   v3 = {1+2+3}
//   v4 = {1} as two bodies   v5 = {1} as two bodies, peeled
// The two-body forms cost registers (kernel-resource-usage: D=128 spills to
// scratch with the in-loop branch, D=64 drops from 4 to 2-3 waves/SIMD),
// which is why v1 masks in place; they are timed for the record.
//
// Gates before any timing: full-tensor BITWISE equality with v0 (all three
// changes are exact-arithmetic no-ops) on tail / one-key-tail / full-tile /
// spiked (forced late rescale) shapes at D=128 and D=64, masked and
// unmasked, and a bitwise double-run race screen per variant.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 attn_v6.hip -o attn_v6
// Run:   ./attn_v6 [rounds]

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <cmath>
#include <type_traits>

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
#define LDS_P __attribute__((address_space(3)))
#define PA_DEV __device__ __forceinline__
#define PA_LOG2E 1.4426950408889634f

PA_DEV bf16 f2bf(float v) { return __float2bfloat16(v); }
PA_DEV f32x16 mfma32x32x16(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
PA_DEV unsigned int cvt_pk_bf16(float lo, float hi) {
    unsigned int r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// the partner half-wave's value of x (lane i <-> lane i^32) without LDS:
// v_permlane32_swap exchanges the upper half of its first operand with the
// lower half of its second, so of the two results one is this lane's own x
// and the other its partner's — which is which depends on the half, and a
// commutative combine does not care.
template <typename F>
PA_DEV float half_swap_combine(float x, F f) {
    const unsigned int u = __float_as_uint(x);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return f(__uint_as_float((unsigned int)r[0]),
             __uint_as_float((unsigned int)r[1]));
}
// one v_mul_f32 the SLP vectorizer cannot pair into v_pk_mul_f32
PA_DEV float mul_scalar(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <int D, int OPT, bool MASKED>
__global__ __launch_bounds__(512, 2) void attn_v6_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, bf16* __restrict__ out,
    int S, int Sk, float scale, int H,
    const unsigned long long* __restrict__ mask_words,
    const int* __restrict__ mask_live, const int* __restrict__ mask_nlive) {
    constexpr bool O_FULL = (OPT & 1) != 0;
    constexpr bool O_SWAP = (OPT & 2) != 0;
    constexpr bool O_SMUL = (OPT & 4) != 0;
    constexpr bool O_TWO = (OPT & 16) != 0 && O_FULL;
    constexpr bool O_PEEL = (OPT & 8) != 0 && O_TWO && !MASKED;
    constexpr int KVBLK = 64;
    constexpr int WAVES = 8;
    constexpr int THREADS = WAVES * 64;
    constexpr int KPAD = D + 8;
    constexpr int VROW = 160;
    constexpr int KK = D / 16;
    constexpr int NV = D / 32;
    constexpr int KVECS = (KVBLK * D) / (8 * THREADS);
    constexpr int DBUF = (D == 128) ? 2 : 1;

    __shared__ bf16 k_lds[DBUF * KVBLK * KPAD];
    __shared__ bf16 v_lds[DBUF * KVBLK * VROW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l32 = lane & 31;
    const int hi = lane >> 5;
    const int trb = (hi * 8 + ((lane & 15) >> 2)) * VROW +
                    16 * (((lane >> 4) & 1) ^ hi) + 4 * (lane & 3);

    const int nq = (S + WAVES * 32 - 1) / (WAVES * 32);
    const long id = blockIdx.x;
    const long bh = (id & 7) + 8 * ((id >> 3) / nq);
    const int qtile = (int)((id >> 3) % nq);
    const long b = bh / H;
    const int h = (int)(bh % H);
    const int q0 = qtile * (WAVES * 32) + wid * 32;
    const int ss = H * D;

    const bf16* qp = q + (b * (long)S) * ss + (long)h * D;
    const bf16* kp = k + (b * (long)Sk) * ss + (long)h * D;
    const bf16* vp = v + (b * (long)Sk) * ss + (long)h * D;
    bf16* op = out + (b * (long)S) * ss + (long)h * D;

    bf16x8 qfrag[KK];
    {
        const int row = q0 + l32;
        const int rr = row < S ? row : (S > 0 ? S - 1 : 0);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
            qfrag[kk] = *reinterpret_cast<const bf16x8*>(
                qp + (long)rr * ss + kk * 16 + hi * 8);
    }

    f32x16 o_acc[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[n][r] = 0.f;
    float m_run = -1e30f, l_run = 0.f;
    const float scale2 = scale * PA_LOG2E;

    bf16x8 kreg[KVECS], vreg[KVECS];
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
                kreg[i] = *reinterpret_cast<const bf16x8*>(
                    kp + (long)src * ss + col);
                vreg[i] = *reinterpret_cast<const bf16x8*>(
                    vp + (long)src * ss + col);
            } else {
                kreg[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                vreg[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
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
            *reinterpret_cast<bf16x8*>(
                &v_lds[buf * (KVBLK * VROW) + row * VROW +
                       (col ^ ((row & 8) << 1))]) = vreg[i];
        }
    };

    auto qk_phase = [&](int buf, f32x16* st) {
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
                st[kt] = mfma32x32x16(afrag, qfrag[kk], st[kt]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };
    // full_c = std::true_type: every key of the tile is live (no per-key
    // work); std::false_type: the shipped per-key test
    auto softmax_phase = [&](auto full_c, int kv0, f32x16* st, bf16x8* pfrag,
                             unsigned long long word) {
        constexpr bool FULL = decltype(full_c)::value;
        float mx = -3e30f;
        if constexpr (FULL) {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[kt][r]);
        } else {
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
                    const float sv = valid ? st[kt][r] : -3e30f;
                    st[kt][r] = sv;
                    mx = fmaxf(mx, sv);
                }
        }
        if constexpr (O_SWAP)
            mx = half_swap_combine(
                mx, [](float a, float c) { return fmaxf(a, c); });
        else
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
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
        if constexpr (O_SWAP)
            ps = half_swap_combine(ps, [](float a, float c) { return a + c; });
        else
            ps += __shfl_xor(ps, 32, 64);
        l_run = l_run * alpha + ps;
        if (alpha != 1.f) {
#pragma unroll
            for (int n = 0; n < NV; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (O_SMUL)
                        o_acc[n][r] = mul_scalar(o_acc[n][r], alpha);
                    else
                        o_acc[n][r] *= alpha;
                }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x16& sv = st[c >> 1];
            const int rb = 8 * (c & 1);
            unsigned int w0 = cvt_pk_bf16(sv[rb + 0], sv[rb + 1]);
            unsigned int w1 = cvt_pk_bf16(sv[rb + 2], sv[rb + 3]);
            unsigned int w2 = cvt_pk_bf16(sv[rb + 4], sv[rb + 5]);
            unsigned int w3 = cvt_pk_bf16(sv[rb + 6], sv[rb + 7]);
            auto r02 = __builtin_amdgcn_permlane32_swap(w0, w2, false, false);
            auto r13 = __builtin_amdgcn_permlane32_swap(w1, w3, false, false);
            unsigned int d[4] = {(unsigned int)r02[0], (unsigned int)r13[0],
                                 (unsigned int)r02[1], (unsigned int)r13[1]};
            pfrag[c] = *reinterpret_cast<bf16x8*>(d);
        }
    };
    // the shipped -3e30 substitution alone, in place on the scores
    auto mask_scores = [&](int kv0, f32x16* st, unsigned long long word) {
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
                const int key = kv0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                bool valid;
                if constexpr (MASKED)
                    valid = ((wh[kt] >> ((r & 3) + 8 * (r >> 2))) & 1u) != 0;
                else
                    valid = key < Sk;
                st[kt][r] = valid ? st[kt][r] : -3e30f;
            }
    };
    // peel_c = std::true_type: the caller guarantees a full tile
    auto softmax_tile = [&](auto peel_c, int tile, f32x16* st, bf16x8* pfrag,
                            unsigned long long word) {
        if constexpr (!O_FULL) {
            softmax_phase(std::false_type{}, tile * KVBLK, st, pfrag, word);
        } else if constexpr (decltype(peel_c)::value) {
            softmax_phase(std::true_type{}, tile * KVBLK, st, pfrag, word);
        } else {
            bool full;
            if constexpr (MASKED) full = word == ~0ull;
            else full = tile * KVBLK + KVBLK <= Sk;
            if constexpr (O_TWO) {
                if (full)
                    softmax_phase(std::true_type{}, tile * KVBLK, st, pfrag,
                                  word);
                else
                    softmax_phase(std::false_type{}, tile * KVBLK, st, pfrag,
                                  word);
            } else {
                if (!full) mask_scores(tile * KVBLK, st, word);
                softmax_phase(std::true_type{}, tile * KVBLK, st, pfrag, word);
            }
        }
    };
    auto pv_phase = [&](int buf, bf16x8* pfrag) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int n = 0; n < NV; ++n) {
                s16x4 alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (LDS_P s16x4*)&v_lds[buf * (KVBLK * VROW) + trb +
                                         c * (16 * VROW) + n * 32]);
                s16x4 ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (LDS_P s16x4*)&v_lds[buf * (KVBLK * VROW) + trb +
                                         c * (16 * VROW) + 4 * VROW + n * 32]);
                bf16x8 va =
                    __builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7);
                o_acc[n] = mfma32x32x16(va, pfrag[c], o_acc[n]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };

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
    if constexpr (DBUF == 2) {
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
        auto body = [&](auto peel_c, int j) {
            const int p = j & 1;
            const int tile = tile_at(j);
            f32x16 st[2];
            bf16x8 pfrag[4];
            qk_phase(p, st);
            if (j + 1 < nt) write_k_lds(p ^ 1);
            softmax_tile(peel_c, tile, st, pfrag, word_of(tile));
            if (j + 1 < nt) write_v_lds(p ^ 1);
            if (j + 2 < nt) {
                const int t2 = tile_at(j + 2);
                issue_tile_loads(t2 * KVBLK, word_of(t2));
            }
            pv_phase(p, pfrag);
            __syncthreads();
        };
        if constexpr (O_PEEL) {
            for (int j = 0; j + 1 < nt; ++j) body(std::true_type{}, j);
            if (nt > 0) body(std::false_type{}, nt - 1);
        } else {
            for (int j = 0; j < nt; ++j) body(std::false_type{}, j);
        }
    } else {
        if (!MASKED || nt > 0) {
            const int t0 = tile_at(0);
            issue_tile_loads(t0 * KVBLK, word_of(t0));
        }
        auto body = [&](auto peel_c, int j) {
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
            softmax_tile(peel_c, tile, st, pfrag, word_of(tile));
            pv_phase(0, pfrag);
        };
        if constexpr (O_PEEL) {
            for (int j = 0; j + 1 < nt; ++j) body(std::true_type{}, j);
            if (nt > 0) body(std::false_type{}, nt - 1);
        } else {
            for (int j = 0; j < nt; ++j) body(std::false_type{}, j);
        }
    }

    const int row = q0 + l32;
    if (row < S) {
        const float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
        for (int n = 0; n < NV; ++n)
#pragma unroll
            for (int r2 = 0; r2 < 4; ++r2) {
                const int dim0 = n * 32 + 8 * r2 + 4 * hi;
                unsigned short pack[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    pack[j] = __bfloat16_as_ushort(
                        f2bf(o_acc[n][r2 * 4 + j] * inv_l));
                *reinterpret_cast<unsigned long long*>(
                    op + (long)row * ss + dim0) =
                    *reinterpret_cast<unsigned long long*>(pack);
            }
    }
}

// ---------------------------------------------------------------------------
#define HIP_CHECK(x) do { hipError_t e = (x); if (e) { \
    printf("HIP error %d at %d\n", e, __LINE__); exit(1); } } while (0)

static void fill_random(bf16* dst, long n, unsigned seed) {
    std::vector<unsigned short> h(1 << 20);
    unsigned x = seed;
    for (auto& e : h) {
        x = x * 1664525u + 1013904223u;
        float f = ((x >> 8) / 8388608.0f) * 2.f - 1.f;
        unsigned int bits;
        __builtin_memcpy(&bits, &f, 4);
        e = (unsigned short)(bits >> 16);
    }
    for (long off = 0; off < n; off += (1 << 20)) {
        long len = std::min<long>(1 << 20, n - off);
        HIP_CHECK(hipMemcpy(dst + off, h.data(), len * 2,
                            hipMemcpyHostToDevice));
    }
}

constexpr int NVAR = 6;
constexpr int VAR_OPT[NVAR] = {0, 1, 3, 7, 17, 25};

// all-true key mask in the packed form the shipped kernel reads: one 64-bit
// word per tile (bits at or beyond Sk clear), the list of live tiles, and
// their count, per batch element
struct Mask {
    unsigned long long* words = nullptr;
    int* live = nullptr;
    int* nlive = nullptr;
};
static Mask make_all_true_mask(int B, int Sk) {
    const int nt = (Sk + 63) / 64;
    std::vector<unsigned long long> w((size_t)B * nt, ~0ull);
    std::vector<int> lv((size_t)B * nt), nl(B, nt);
    for (int b = 0; b < B; ++b) {
        for (int t = 0; t < nt; ++t) lv[(size_t)b * nt + t] = t;
        if (Sk % 64) w[(size_t)b * nt + nt - 1] = (1ull << (Sk % 64)) - 1;
    }
    Mask m;
    HIP_CHECK(hipMalloc(&m.words, w.size() * 8));
    HIP_CHECK(hipMalloc(&m.live, lv.size() * 4));
    HIP_CHECK(hipMalloc(&m.nlive, nl.size() * 4));
    HIP_CHECK(hipMemcpy(m.words, w.data(), w.size() * 8,
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(m.live, lv.data(), lv.size() * 4,
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(m.nlive, nl.data(), nl.size() * 4,
                        hipMemcpyHostToDevice));
    return m;
}
static void free_mask(Mask& m) {
    (void)hipFree(m.words); (void)hipFree(m.live); (void)hipFree(m.nlive);
}

template <int D, int OPT>
static void launch_opt(const bf16* q, const bf16* k, const bf16* v, bf16* o,
                       int B, int H, int S, float scale, const Mask* m) {
    dim3 grid(((S + 255) / 256) * B * H), blk(512);
    if (m)
        hipLaunchKernelGGL((attn_v6_kernel<D, OPT, true>), grid, blk, 0, 0, q,
                           k, v, o, S, S, scale, H, m->words, m->live,
                           m->nlive);
    else
        hipLaunchKernelGGL((attn_v6_kernel<D, OPT, false>), grid, blk, 0, 0,
                           q, k, v, o, S, S, scale, H, nullptr, nullptr,
                           nullptr);
}

template <int D>
static void launch(int var, const bf16* q, const bf16* k, const bf16* v,
                   bf16* o, int B, int H, int S, float scale, const Mask* m) {
    switch (var) {
    case 0: launch_opt<D, VAR_OPT[0]>(q, k, v, o, B, H, S, scale, m); break;
    case 1: launch_opt<D, VAR_OPT[1]>(q, k, v, o, B, H, S, scale, m); break;
    case 2: launch_opt<D, VAR_OPT[2]>(q, k, v, o, B, H, S, scale, m); break;
    case 3: launch_opt<D, VAR_OPT[3]>(q, k, v, o, B, H, S, scale, m); break;
    case 4: launch_opt<D, VAR_OPT[4]>(q, k, v, o, B, H, S, scale, m); break;
    default: launch_opt<D, VAR_OPT[5]>(q, k, v, o, B, H, S, scale, m);
    }
}

// spike: 0 none; 1 a K row of 10.0 in the last full tile; 2 in the last
// tile (the partial tail when S % 64 != 0) — both force alpha != 1 late
template <int D>
static int check_correct(int B, int H, int S, int spike, bool masked) {
    const long n = (long)B * S * H * D;
    bf16 *q, *k, *v, *o;
    HIP_CHECK(hipMalloc(&q, n * 2));
    HIP_CHECK(hipMalloc(&k, n * 2));
    HIP_CHECK(hipMalloc(&v, n * 2));
    HIP_CHECK(hipMalloc(&o, n * 2));
    fill_random(q, n, 1234);
    fill_random(k, n, 777);
    fill_random(v, n, 4242);
    if (spike) {
        const int full_tiles = S / 64;
        const int row = spike == 1 ? (full_tiles > 0 ? full_tiles * 64 - 7 : 0)
                                   : S - 1;
        std::vector<unsigned short> big(H * D, 0x4120);  // 10.0 bf16
        HIP_CHECK(hipMemcpy(k + (long)row * H * D, big.data(),
                            big.size() * 2, hipMemcpyHostToDevice));
    }
    Mask mk;
    if (masked) mk = make_all_true_mask(B, S);
    const Mask* m = masked ? &mk : nullptr;
    const float scale = 1.0f / sqrtf((float)D);
    std::vector<unsigned short> ref(n), got(n), got2(n);
    launch<D>(0, q, k, v, o, B, H, S, scale, m);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(ref.data(), o, n * 2, hipMemcpyDeviceToHost));
    int fails = 0;
    for (int var = 1; var < NVAR; ++var) {
        HIP_CHECK(hipMemset(o, 0, n * 2));
        launch<D>(var, q, k, v, o, B, H, S, scale, m);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(got.data(), o, n * 2, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemset(o, 0, n * 2));
        launch<D>(var, q, k, v, o, B, H, S, scale, m);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(got2.data(), o, n * 2, hipMemcpyDeviceToHost));
        long bad = 0, race = 0;
        for (long i = 0; i < n; ++i) {
            if (got[i] != got2[i]) ++race;
            if (got[i] != ref[i]) ++bad;  // exact no-ops: bitwise or wrong
        }
        if (bad || race) {
            printf("VAR %d (opt %d) WRONG D=%d S=%d spike=%d masked=%d: "
                   "%ld/%ld differ from v0, %ld race\n", var, VAR_OPT[var], D,
                   S, spike, (int)masked, bad, n, race);
            ++fails;
        }
    }
    if (masked) free_mask(mk);
    (void)hipFree(q); (void)hipFree(k); (void)hipFree(v); (void)hipFree(o);
    return fails;
}

template <int D>
static int check_all() {
    int fails = 0;
    // B*H must be a multiple of 8 (XCD-affine block decode). S=1000: 40-key
    // tail; 961: one-key tail; 1024: full tiles only; 40: only a partial tile
    const int sizes[4] = {1000, 961, 1024, 40};
    for (int s : sizes)
        for (int masked = 0; masked < 2; ++masked)
            for (int spike = 0; spike < 3; ++spike)
                fails += check_correct<D>(2, 4, s, spike, masked != 0);
    return fails;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 8;
    int fails = check_all<128>() + check_all<64>();
    if (fails) { printf("CORRECTNESS FAILED (%d)\n", fails); return 1; }
    printf("correctness: all variants bitwise equal to v0 "
           "(tails + full + spikes + masked + race screen)\n");

    struct Shape { int B, H, S, D; bool masked; const char* name; };
    Shape shapes[4] = {{8, 24, 4608, 128, false, "flux"},
                       {1, 8, 30720, 128, false, "long"},
                       {8, 38, 4250, 64, false, "sd3-d64"},
                       {8, 24, 4608, 128, true, "flux-msk"}};
    for (auto& sh : shapes) {
        const int B = sh.B, H = sh.H, S = sh.S, D = sh.D;
        const long n = (long)B * S * H * D;
        bf16 *q, *k, *v, *o;
        HIP_CHECK(hipMalloc(&q, n * 2));
        HIP_CHECK(hipMalloc(&k, n * 2));
        HIP_CHECK(hipMalloc(&v, n * 2));
        HIP_CHECK(hipMalloc(&o, n * 2));
        fill_random(q, n, 12345);
        fill_random(k, n, 54321);
        fill_random(v, n, 999);
        Mask mk;
        if (sh.masked) mk = make_all_true_mask(B, S);
        const Mask* m = sh.masked ? &mk : nullptr;
        const float scale = 1.0f / sqrtf((float)D);
        const double tf = 4.0 * B * H * (double)S * S * D / 1e12;
        double best[NVAR], worst[NVAR];
        for (auto& x : best) x = 1e30;
        for (auto& x : worst) x = 0;
        auto run = [&](int var) {
            if (D == 64)
                launch<64>(var, q, k, v, o, B, H, S, scale, m);
            else
                launch<128>(var, q, k, v, o, B, H, S, scale, m);
        };
        for (int var = 0; var < NVAR; ++var) run(var);
        HIP_CHECK(hipDeviceSynchronize());
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        for (int r = 0; r < rounds; ++r)
            for (int var = 0; var < NVAR; ++var) {
                HIP_CHECK(hipEventRecord(e0));
                for (int it = 0; it < 3; ++it) run(var);
                HIP_CHECK(hipEventRecord(e1));
                HIP_CHECK(hipEventSynchronize(e1));
                float ms;
                HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
                best[var] = std::min(best[var], ms / 3.0);
                worst[var] = std::max(worst[var], ms / 3.0);
            }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        // best and worst round per variant: a win counts when a variant's
        // worst round beats v0's best
        printf("%-8s", sh.name);
        for (int var = 0; var < NVAR; ++var)
            printf("  v%d %7.3f..%7.3f ms (%6.1f TF)", var, best[var],
                   worst[var], tf / best[var] * 1e3);
        printf("\n");
        if (sh.masked) free_mask(mk);
        (void)hipFree(q); (void)hipFree(k); (void)hipFree(v); (void)hipFree(o);
    }
    return 0;
}
