// Top-p tile selector for per-head block-sparse attention: block means of q
// and k, then per (b, h, query block) the smallest set of key tiles whose
// softmax mass over the pooled scores reaches top_p. Two kernels, no host
// read, so select -> pack_head_block_lists -> attention captures into one
// graph. docs/KERNELS.md, "Per-head block masks and the top-p selector".
#pragma once

// Tiles a select block can hold: (SEL_QPB + 1) fp32 rows of nk in dynamic LDS,
// 61 440 bytes at the cap, inside the 64 KiB a kernel gets without asking.
// 3072 tiles are 196 608 keys (WAN 720p x 21 frames has 1182).
static constexpr int SEL_QPB = 4;       // query blocks per select block
static constexpr int SEL_NK_CAP = 3072;

// ---------------------------------------------------------------------------
// Pooling pass: x [B, S, H, D] or [B, H, S, D] through strides, 16-bit ->
// mean over each block of R rows (256 for q, 64 for k; the last block over
// its rows < S only), fp32 [B, H, n, D], n = ceil(S / R).
//
// One 256-thread block per (row block, h, b). A row is D/8 16-byte granules;
// thread t owns granule t % G of the rows t / G, t / G + 256 / G, ... (G = 8
// or 16), so the G threads of a row read its D * 2 bytes contiguously, once,
// in place. Eight fp32 sums per thread in registers (constant indices), one
// LDS transpose [256 / G][D] (8 KiB) to add the 256 / G row lanes in a fixed
// order, and thread c < D writes column c. Memory-bound: q and k are read
// exactly once.
// ---------------------------------------------------------------------------
template <int D, typename E>
__global__ __launch_bounds__(256) void pool_rows_kernel(
    const E* __restrict__ x, float* __restrict__ out, int S, int R, int n,
    long x_bs, long x_hs, long x_ss) {
    using EL = Elem16<E>;
    constexpr int G = D / 8;          // granules per row
    constexpr int RL = 256 / G;       // row lanes
    __shared__ float part[RL * D];
    const int blk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int H = gridDim.y;
    const int g = threadIdx.x % G, rl = threadIdx.x / G;
    const int r0 = blk * R;
    const int rows = min(R, S - r0);
    const E* xp = x + b * x_bs + h * x_hs + (long)r0 * x_ss + g * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = rl; r < rows; r += RL) {
        const short8 v = *reinterpret_cast<const short8*>(xp + (long)r * x_ss);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += EL::ld((unsigned short)v[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[rl * D + g * 8 + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < D) {
        float s = 0.f;
#pragma unroll 8
        for (int i = 0; i < RL; ++i) s += part[i * D + threadIdx.x];
        out[(((long)b * H + h) * n + blk) * D + threadIdx.x] =
            s / (float)rows;
    }
}

// x: 4-D 16-bit, bshd or bhsd; returns fp32 [B, H, ceil(S / R), D].
static at::Tensor pool_rows(const at::Tensor& x, bool bshd, int R) {
    const int s_ax = bshd ? 1 : 2, h_ax = bshd ? 2 : 1;
    const int B = (int)x.size(0), S = (int)x.size(s_ax),
              H = (int)x.size(h_ax), D = (int)x.size(3);
    // as the head dims below their class in attn_fwd: the op exists to read
    // views in place, so a row start off 16 bytes is refused, not copied
    TORCH_CHECK(x.stride(3) == 1 && (x.stride(s_ax) % 8) == 0 &&
                    (x.stride(h_ax) % 8) == 0 && (x.stride(0) % 8) == 0 &&
                    (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0,
                "select_block_mask: every row of q/k must start on 16 bytes "
                "(base aligned, last dim contiguous, all other strides "
                "multiples of 8 elements), got strides ", x.strides());
    const int n = (S + R - 1) / R;
    auto out = at::empty({B, H, n, D}, x.options().dtype(at::kFloat));
    if (out.numel() == 0) return out;
    const dim3 grid((unsigned)n, (unsigned)H, (unsigned)B);
#define PA_POOL(D_)                                                          \
    PA_WITH_ELEM16(x.scalar_type(), hipLaunchKernelGGL(                      \
        HIP_KERNEL_NAME(pool_rows_kernel<D_, E>), grid, dim3(256), 0,        \
        cur_stream(), (const E*)x.data_ptr(), out.data_ptr<float>(), S, R,   \
        n, (long)x.stride(0), (long)x.stride(h_ax), (long)x.stride(s_ax)))
    if (D == 64) PA_POOL(64);
    else PA_POOL(128);
#undef PA_POOL
    return out;
}

// Order-preserving image of a finite fp32 in the unsigned integers: a < b as
// floats iff sel_key(a) < sel_key(b) (-0 is made +0 first, so equal floats
// have equal keys).
PA_DEV unsigned int sel_key(float s) {
    const unsigned int u = __float_as_uint(s + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int BLOCK>
PA_DEV float block_reduce_max(float v, float* scratch) {
    constexpr int NW = BLOCK / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, 64));
    __syncthreads();  // protect scratch against the previous reduction's reads
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    float total = scratch[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) total = fmaxf(total, scratch[i]);
    return total;
}

// ---------------------------------------------------------------------------
// Select pass: qbar [B, H, nq, D], kbar [B, H, nk, D] fp32 -> mask [B, H, nq,
// nk] bytes, 1 = tile t selected for query block qb:
//   s_t = scale * <qbar, kbar_t>,  p_t = exp(s_t - max s),  Z = sum p
//   selected iff  sum of p_u over { u : s_u > s_t }  <  top_p * Z
// (the shortest descending prefix reaching top_p, ties at the threshold all
// kept), OR keep[qb][t].
//
// Work split. One 256-thread block owns QPB consecutive query blocks of one
// (b, h), so the head's kbar (605 KB at WAN 720p x 21) is read once per QPB
// query blocks, not once per query block. Scores: 16 lanes share a tile, lane
// l holding columns 64 c + 4 l .. + 3 of the kbar row (one or two float4
// loads, the 16 lanes reading the row's 256 or 512 bytes contiguously)
// against the same columns of the QPB qbar rows, which sit in QPB * D / 16
// registers for the whole pass (constant indices); a 4-step xor shuffle adds
// the 16 partial dots, lane 0 of the group stores the score. A block covers
// 16 tiles per step. Scores of the QPB query blocks fill QPB rows of nk
// floats in LDS.
//
// Threshold, per query block in turn: block max, then p into a further LDS
// row with the normaliser, then a bisection over sel_key's integers for
//   x* = min { x : sum of p_u over { u : key_u > x } < top_p * Z },
// 32 steps, each a block-wide masked sum of p in a fixed order (every thread
// adds its own tiles tid, tid + 256, ..., a shuffle tree per wave, the four
// wave sums in order). fp32 addition is monotone, so the masked sum is a
// nonincreasing function of x in floating point too and the bisection finds
// x* exactly: tile t is selected iff key_t >= x*. No sort, no atomics, the
// same bits on every run. Nothing is indexed at run time but LDS and global
// memory: no scratch.
// ---------------------------------------------------------------------------
template <int D, int QPB>
__global__ __launch_bounds__(256) void select_tiles_kernel(
    const float* __restrict__ qbar, const float* __restrict__ kbar,
    const unsigned char* __restrict__ keep, unsigned char* __restrict__ mask,
    int nq, int nk, float scale, float top_p) {
    constexpr int NV = D / 64;        // float4 loads per lane and row
    extern __shared__ float sel_lds[];    // [QPB][nk] scores, then [nk] p
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int sub = tid & 15, grp = tid >> 4;
    const int g0 = blockIdx.x * QPB;
    const long bh = (long)blockIdx.z * gridDim.y + blockIdx.y;

    float4 qv[QPB][NV];
#pragma unroll
    for (int i = 0; i < QPB; ++i) {
        const int qb = min(g0 + i, nq - 1);
#pragma unroll
        for (int c = 0; c < NV; ++c)
            qv[i][c] = *reinterpret_cast<const float4*>(
                qbar + (bh * nq + qb) * D + c * 64 + sub * 4);
    }
    const float* kb = kbar + bh * nk * D + sub * 4;
    for (int base = 0; base < nk; base += 16) {
        // every lane of the wave takes every trip (the shuffles below), the
        // groups past the end on the last tile again
        const int t = base + grp;
        const float* kr = kb + (long)min(t, nk - 1) * D;
        float4 kv[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c)
            kv[c] = *reinterpret_cast<const float4*>(kr + c * 64);
        float dot[QPB];
#pragma unroll
        for (int i = 0; i < QPB; ++i) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < NV; ++c)
                d += qv[i][c].x * kv[c].x + qv[i][c].y * kv[c].y +
                     qv[i][c].z * kv[c].z + qv[i][c].w * kv[c].w;
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
            dot[i] = d;
        }
        if (sub == 0 && t < nk) {
#pragma unroll
            for (int i = 0; i < QPB; ++i) sel_lds[i * nk + t] = dot[i] * scale;
        }
    }
    float* p = sel_lds + QPB * nk;
#pragma unroll 1
    for (int i = 0; i < QPB; ++i) {
        const int qb = g0 + i;
        if (qb >= nq) break;              // block-uniform
        const float* s = sel_lds + i * nk;
        __syncthreads();                  // scores written; p of qb - 1 read
        float m = -INFINITY;
        for (int t = tid; t < nk; t += 256) m = fmaxf(m, s[t]);
        m = block_reduce_max<256>(m, red);
        float z = 0.f;
        for (int t = tid; t < nk; t += 256) {
            const float e = __expf(s[t] - m);
            p[t] = e;                     // read back by this thread only
            z += e;
        }
        z = block_reduce_sum<256>(z, red);
        const float theta = top_p * z;
        // invariant: mass above hi < theta (nothing lies above 0xffffffff)
        unsigned int lo = 0u, hi = 0xffffffffu;
#pragma unroll 1
        for (int step = 0; step < 32 && lo < hi; ++step) {
            const unsigned int mid = lo + ((hi - lo) >> 1);
            float a = 0.f;
            for (int t = tid; t < nk; t += 256)
                a += sel_key(s[t]) > mid ? p[t] : 0.f;
            a = block_reduce_sum<256>(a, red);
            if (a < theta) hi = mid;
            else lo = mid + 1u;
        }
        unsigned char* mrow = mask + (bh * nq + qb) * nk;
        const unsigned char* krow = keep ? keep + (long)qb * nk : nullptr;
        for (int t = tid; t < nk; t += 256)
            mrow[t] = (sel_key(s[t]) >= hi || (krow && krow[t] != 0)) ? 1 : 0;
    }
}

// q, k: 4-D bf16/fp16 of head dim 64 or 128, [B, S, H, D] (bshd) or [B, H, S,
// D], any 16-byte-aligned strided views. keep: optional bool [nq, nk].
// Returns bool [B, H, ceil(Sq/256), ceil(Sk/64)].
at::Tensor select_block_mask(at::Tensor q, at::Tensor k, double top_p,
                             double scale, bool bshd,
                             c10::optional<at::Tensor> keep) {
    CHECK_GPU(q);
    TORCH_CHECK(is_elem16(q.scalar_type()),
                "select_block_mask: bf16 or fp16 only, got ", q.scalar_type());
    CHECK_SAME_DTYPE(k, q);
    CHECK_SAME_DEVICE(k, q);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4,
                "select_block_mask expects 4-D q/k");
    const int s_ax = bshd ? 1 : 2, h_ax = bshd ? 2 : 1;
    const long B = q.size(0), H = q.size(h_ax), D = q.size(3);
    TORCH_CHECK(D == 64 || D == 128,
                "select_block_mask: head dim 64 or 128, got ", D);
    TORCH_CHECK(k.size(0) == B && k.size(h_ax) == H && k.size(3) == D,
                "select_block_mask: k must have q's batch, heads and head "
                "dim, got q ", q.sizes(), ", k ", k.sizes());
    TORCH_CHECK(top_p > 0.0 && top_p < 1.0,
                "select_block_mask: top_p inside (0, 1) (1 needs no kernel), "
                "got ", top_p);
    TORCH_CHECK(B <= 65535 && H <= 65535,
                "select_block_mask: batch or heads exceed 65535");
    const long Sq = q.size(s_ax), Sk = k.size(s_ax);
    const long nq = (Sq + 255) / 256, nk = (Sk + 63) / 64;
    TORCH_CHECK(nk <= SEL_NK_CAP, "select_block_mask: ", nk, " key tiles "
                "exceed the LDS cap of ", SEL_NK_CAP, " (", SEL_NK_CAP * 64,
                " keys)");
    const unsigned char* keep_p = nullptr;
    at::Tensor keep_c;
    if (keep.has_value()) {
        CHECK_SAME_DEVICE(*keep, q);
        TORCH_CHECK(keep->scalar_type() == at::kBool && keep->dim() == 2 &&
                        keep->size(0) == nq && keep->size(1) == nk,
                    "select_block_mask: keep must be bool [", nq, ", ", nk,
                    "], got ", keep->scalar_type(), " ", keep->sizes());
        keep_c = keep->contiguous();
        keep_p = (const unsigned char*)keep_c.data_ptr();
    }
    auto mask = at::empty({B, H, nq, nk}, q.options().dtype(at::kBool));
    if (mask.numel() == 0) return mask;
    const auto qbar = pool_rows(q, bshd, 256);
    const auto kbar = pool_rows(k, bshd, 64);
    const dim3 grid((unsigned)((nq + SEL_QPB - 1) / SEL_QPB), (unsigned)H,
                    (unsigned)B);
    const size_t lds = (size_t)(SEL_QPB + 1) * nk * sizeof(float);
#define PA_SELECT(D_)                                                        \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(select_tiles_kernel<D_, SEL_QPB>),    \
                       grid, dim3(256), lds, cur_stream(),                   \
                       qbar.data_ptr<float>(), kbar.data_ptr<float>(),       \
                       keep_p, (unsigned char*)mask.data_ptr(), (int)nq,     \
                       (int)nk, (float)scale, (float)top_p)
    if (D == 64) PA_SELECT(64);
    else PA_SELECT(128);
#undef PA_SELECT
    return mask;
}
