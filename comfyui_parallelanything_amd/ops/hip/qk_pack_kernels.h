// Kernels of the fused qk RMSNorm + RoPE (in place) and of the dual-stream
// joint qkv pack. Device code only: it needs PA_DEV, short8, Elem16 and
// wave_reduce_sum (common.h) and nothing of torch, so scripts/qknr_ab.hip
// compiles this same text beside a few lines of its own.
#pragma once

// One lane's share of "RMSNorm over D, per-dim weight, rotate by (c, s)" for
// the pair packed in u; returns the packed result. The sum of squares is a
// 64-lane reduction, so EVERY lane of the wave must call this: a lane with
// no pair (act == false, D < 128) contributes 0 and discards the result.
template <typename EL>
PA_DEV unsigned int rms_rope_pair(unsigned int u, float w0, float w1, float c,
                                  float s, bool act, int D, float eps) {
    float a0 = EL::ld((unsigned short)(u & 0xffff));
    float a1 = EL::ld((unsigned short)(u >> 16));
    const float ss = wave_reduce_sum(act ? a0 * a0 + a1 * a1 : 0.f);
    const float rr = rsqrtf(ss / (float)D + eps);
    a0 = a0 * rr * w0;
    a1 = a1 * rr * w1;
    return (unsigned int)EL::st(a0 * c - a1 * s) |
           ((unsigned int)EL::st(a0 * s + a1 * c) << 16);
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
        const unsigned int oq = rms_rope_pair<EL>(
            uq[i], wq0, wq1, cvec[i], svec[i], act, D, eps);
        if (act) qp[i][lane] = oq;
        const unsigned int ok = rms_rope_pair<EL>(
            uk[i], wk0, wk1, cvec[i], svec[i], act, D, eps);
        if (act) kp[i][lane] = ok;
    }
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
        const unsigned int rq = rms_rope_pair<EL>(
            uq[i], EL::ld((unsigned short)(uwq[i] & 0xffff)),
            EL::ld((unsigned short)(uwq[i] >> 16)), cvec[i], svec[i], act, D,
            eps);
        if (act) reinterpret_cast<unsigned int*>(oq)[obase[i] + lane] = rq;
        const unsigned int rk = rms_rope_pair<EL>(
            uk[i], EL::ld((unsigned short)(uwk[i] & 0xffff)),
            EL::ld((unsigned short)(uwk[i] >> 16)), cvec[i], svec[i], act, D,
            eps);
        if (act) reinterpret_cast<unsigned int*>(ok)[obase[i] + lane] = rk;
        if (act) reinterpret_cast<unsigned int*>(ov)[obase[i] + lane] = uv[i];
    }
}

// ---------------------------------------------------------------------------
// Token-major fast path of both ops, for D = 128 or 64 with the heads of a
// token contiguous (head stride == D) and every base and stride a multiple of
// 16 bytes. A token's q (and k, v) is then one run of H * D elements. One
// lane holds 8 consecutive elements (one 16-byte load and store), DT / 8
// lanes hold a row, a wave instruction covers 512 elements = 512 / DT whole
// rows, and a wave walks CH such instructions of one token. 512 is a
// multiple of DT, so a lane keeps its place in the row for every head: the
// norm weights and the token's cos/sin pairs are loaded once per wave, and
// the only index arithmetic is one 32-bit (wave -> token, chunk) split.
//
// The result is bit for bit that of the kernels above. They reduce
// p[i] = a0 * a0 + a1 * a1 over the pair index i with xor-butterflies of
// 32, 16, 8, 4, 2, 1: a balanced tree over the bits of i, high bit first.
// Here lane l of a row holds the pairs i = 4 l + j (j = 0..3), so bits 5..2
// of i are l and the first four levels are lane-xors of 8, 4, 2, 1 applied
// to each of the four partials t[j]; bits 1 and 0 are j, so the tree ends in
// (t[0] + t[2]) + (t[1] + t[3]) inside the lane. At D = 64 the kernels
// above add exact zeros at their first level (lanes 32..63 hold none), so
// the 8-lane rows start at lane-xor 4. The leaf, the division by the runtime
// D, rsqrtf and the rotation are the expressions of rms_rope_pair, with the
// contraction pinned to what those compile to (rms_rope_vec8).
// ---------------------------------------------------------------------------

// v of lane (l ^ M) inside a 16-lane row, M in {8, 4, 2, 1}. kDpp: DPP moves
// (row_ror:8 is l ^ 8 in a row of 16; quad_perm for 2 and 1) and one
// ds_swizzle for 4, none of which needs an address register; else
// __shfl_xor. Every lane of the row must be active.
template <int M, bool kDpp>
PA_DEV float row_xor(float v) {
    if constexpr (!kDpp) {
        return __shfl_xor(v, M, 64);
    } else {
        int i = __builtin_bit_cast(int, v);
        if constexpr (M == 8)
            i = __builtin_amdgcn_update_dpp(0, i, 0x128, 0xf, 0xf, true);
        else if constexpr (M == 4)
            i = __builtin_amdgcn_ds_swizzle(i, (4 << 10) | 0x1f);
        else if constexpr (M == 2)
            i = __builtin_amdgcn_update_dpp(0, i, 0x4e, 0xf, 0xf, true);
        else
            i = __builtin_amdgcn_update_dpp(0, i, 0xb1, 0xf, 0xf, true);
        return __builtin_bit_cast(float, i);
    }
}

// Eight floats of a 16-bit vector.
template <typename EL>
PA_DEV void ld8(short8 u, float (&f)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = EL::ld((unsigned short)u[j]);
}

// rms_rope_pair for the four pairs in u; w and cs are this lane's eight
// weights and four (cos, sin) pairs. Every lane of the row must call it.
template <typename EL, int DT, bool kDpp>
PA_DEV short8 rms_rope_vec8(short8 u, const float (&w)[8],
                            const float (&cs)[8], int D, float eps) {
    // The kernels above compile to packed multiplies followed by a plain
    // add or subtract, for the leaf and for the rotation alike (the packing
    // comes before the contraction would); with four pairs in a lane the
    // compiler contracts the same text into v_pk_fma_f32, one rounding
    // fewer, and 1e-5 of the outputs differ in their last bit. Pinned.
#pragma clang fp contract(off)
    float a[8], t[4];
    ld8<EL>(u, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a0 = a[2 * j], a1 = a[2 * j + 1];
        t[j] = a0 * a0 + a1 * a1;
    }
    if constexpr (DT == 128) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] += row_xor<8, kDpp>(t[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] += row_xor<4, kDpp>(t[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] += row_xor<2, kDpp>(t[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] += row_xor<1, kDpp>(t[j]);
    const float ss = (t[0] + t[2]) + (t[1] + t[3]);
    const float rr = rsqrtf(ss / (float)D + eps);
    short8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a0 = a[2 * j], a1 = a[2 * j + 1];
        const float c = cs[2 * j], s = cs[2 * j + 1];
        a0 = a0 * rr * w[2 * j];
        a1 = a1 * rr * w[2 * j + 1];
        o[2 * j] = (short)EL::st(a0 * c - a1 * s);
        o[2 * j + 1] = (short)EL::st(a0 * s + a1 * c);
    }
    return o;
}

// This lane's four (cos, sin) pairs of table row s: two 16-byte loads.
template <int DT>
PA_DEV void ld_cs8(const float* __restrict__ cs, unsigned s, int pos,
                   float (&f)[8]) {
    const float4* p =
        reinterpret_cast<const float4*>(cs + (long)s * DT + pos);
    const float4 x = p[0], y = p[1];
    f[0] = x.x; f[1] = x.y; f[2] = x.z; f[3] = x.w;
    f[4] = y.x; f[5] = y.y; f[6] = y.z; f[7] = y.w;
}

template <typename E, int DT, int CH, bool kDpp>
__global__ void __launch_bounds__(256)
qk_norm_rope_tok_kernel(E* __restrict__ q, E* __restrict__ k,
                        const E* __restrict__ wq, const E* __restrict__ wk,
                        const float* __restrict__ cs,
                        unsigned S, int HD, int D, long q_bs, long q_ss,
                        long k_bs, long k_ss, unsigned nchunk,
                        unsigned n_work, float eps) {
    using EL = Elem16<E>;
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(
        blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (wave >= n_work) return;
    const unsigned tok = wave / nchunk, chunk = wave % nchunk;
    const unsigned b = tok / S, s = tok % S;
    const int pos = (lane * 8) % DT;        // place in the row, every head
    const int first = (int)chunk * (CH * 512);
    E* qt = q + b * q_bs + s * q_ss;
    E* kt = k + b * k_bs + s * k_ss;

    short8 uq[CH], uk[CH];
    int off[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        // a row past the token's end loads the token's first row instead,
        // stays in the exchanges and skips the store
        const int o = first + i * 512 + lane * 8;
        off[i] = o < HD ? o : -1;
        const int ol = o < HD ? o : pos;
        uq[i] = *reinterpret_cast<const short8*>(qt + ol);
        uk[i] = *reinterpret_cast<const short8*>(kt + ol);
    }
    float fwq[8], fwk[8], fcs[8];
    ld8<EL>(*reinterpret_cast<const short8*>(wq + pos), fwq);
    ld8<EL>(*reinterpret_cast<const short8*>(wk + pos), fwk);
    ld_cs8<DT>(cs, s, pos, fcs);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if (first + i * 512 >= HD) break;   // wave-uniform
        const short8 oq = rms_rope_vec8<EL, DT, kDpp>(uq[i], fwq, fcs, D, eps);
        if (off[i] >= 0) *reinterpret_cast<short8*>(qt + off[i]) = oq;
        const short8 ok = rms_rope_vec8<EL, DT, kDpp>(uk[i], fwk, fcs, D, eps);
        if (off[i] >= 0) *reinterpret_cast<short8*>(kt + off[i]) = ok;
    }
}

template <typename E, int DT, int CH, bool kDpp>
__global__ void __launch_bounds__(256)
pack_joint_qkv_tok_kernel(
    const E* __restrict__ txt, const E* __restrict__ img,
    const E* __restrict__ wq_t, const E* __restrict__ wk_t,
    const E* __restrict__ wq_i, const E* __restrict__ wk_i,
    const float* __restrict__ cs,                   // [T+Si][D/2][2]
    E* __restrict__ oq, E* __restrict__ ok, E* __restrict__ ov,
    unsigned T, unsigned S, int HD, int D,
    long t_bs, long t_ss, long t_qs,                // txt strides (b, s, qkv)
    long i_bs, long i_ss, long i_qs,
    unsigned nchunk, unsigned n_work, float eps) {
    using EL = Elem16<E>;
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(
        blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (wave >= n_work) return;
    const unsigned tok = wave / nchunk, chunk = wave % nchunk;
    const unsigned b = tok / S, s = tok % S;
    const bool is_txt = s < T;
    const int pos = (lane * 8) % DT;
    const int first = (int)chunk * (CH * 512);
    const E* src = is_txt ? txt + b * t_bs + s * t_ss
                          : img + b * i_bs + (s - T) * i_ss;
    const long qs = is_txt ? t_qs : i_qs;
    const long obase = (long)tok * HD;

    short8 uq[CH], uk[CH], uv[CH];
    int off[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int o = first + i * 512 + lane * 8;
        off[i] = o < HD ? o : -1;
        const int ol = o < HD ? o : pos;
        uq[i] = *reinterpret_cast<const short8*>(src + ol);
        uk[i] = *reinterpret_cast<const short8*>(src + qs + ol);
        uv[i] = *reinterpret_cast<const short8*>(src + 2 * qs + ol);
    }
    float fwq[8], fwk[8], fcs[8];
    ld8<EL>(*reinterpret_cast<const short8*>((is_txt ? wq_t : wq_i) + pos),
            fwq);
    ld8<EL>(*reinterpret_cast<const short8*>((is_txt ? wk_t : wk_i) + pos),
            fwk);
    ld_cs8<DT>(cs, s, pos, fcs);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if (first + i * 512 >= HD) break;   // wave-uniform
        const short8 rq = rms_rope_vec8<EL, DT, kDpp>(uq[i], fwq, fcs, D, eps);
        const short8 rk = rms_rope_vec8<EL, DT, kDpp>(uk[i], fwk, fcs, D, eps);
        if (off[i] >= 0) {
            *reinterpret_cast<short8*>(oq + obase + off[i]) = rq;
            *reinterpret_cast<short8*>(ok + obase + off[i]) = rk;
            *reinterpret_cast<short8*>(ov + obase + off[i]) = uv[i];
        }
    }
}
