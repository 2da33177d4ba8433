// Fused qk RMSNorm + RoPE (in place) and the dual-stream joint qkv pack.
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

// What both launchers below ask of a rotary table and a norm weight before
// the kernel indexes them by (s, pair) and by pair.
static void check_cs_table(const char* op, const at::Tensor& cs, long S, long D,
                           const at::Tensor& ref) {
    TORCH_CHECK(cs.dim() == 3 && cs.size(0) == S && cs.size(1) == D / 2 &&
                cs.size(2) == 2, op, ": cs must be [S, D/2, 2] = [", S, ", ",
                D / 2, ", 2], got ", cs.sizes());
    TORCH_CHECK(cs.device() == ref.device(), op, ": cs is on ", cs.device(),
                ", the activations on ", ref.device());
}

static void check_norm_weight(const char* op, const char* name,
                              const at::Tensor& w, long D,
                              const at::Tensor& ref) {
    TORCH_CHECK(w.dim() == 1 && w.size(0) == D, op, ": ", name,
                " must be [D] = [", D, "], got ", w.sizes());
    TORCH_CHECK(w.scalar_type() == ref.scalar_type(), op, ": ", name,
                " dtype (", w.scalar_type(), ") must match the activations (",
                ref.scalar_type(), ")");
    TORCH_CHECK(w.device() == ref.device(), op, ": ", name, " is on ",
                w.device(), ", the activations on ", ref.device());
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

void qk_norm_rope_(at::Tensor q, at::Tensor k, at::Tensor wq, at::Tensor wk,
                   at::Tensor cs, double eps) {
    CHECK_GPU(q);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "qk_norm_rope_: [B,S,H,D] views");
    TORCH_CHECK(is_elem16(q.scalar_type()),
                "qk_norm_rope_: bf16 or fp16 only, got ", q.scalar_type());
    CHECK_SAME_DTYPE(k, q);
    CHECK_SAME_DEVICE(k, q);
    const int B = (int)q.size(0), S = (int)q.size(1), H = (int)q.size(2),
              D = (int)q.size(3);
    TORCH_CHECK(D % 2 == 0 && D <= 128, "qk_norm_rope_: D must be even, <=128");
    TORCH_CHECK(k.sizes() == q.sizes(), "qk_norm_rope_: k ", k.sizes(),
                " must have q's shape ", q.sizes());
    check_norm_weight("qk_norm_rope_", "wq", wq, D, q);
    check_norm_weight("qk_norm_rope_", "wk", wk, D, q);
    check_cs_table("qk_norm_rope_", cs, S, D, q);
    const long rows = (long)B * S * H;
    if (rows == 0 || D == 0) return;
    TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1,
                "qk_norm_rope_: last dim contiguous");
    auto csf = cs.to(at::kFloat).contiguous();
    auto wqc = wq.contiguous();
    auto wkc = wk.contiguous();
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
    CHECK_SAME_DEVICE(img_qkv, txt_qkv);
    const int B = (int)txt_qkv.size(0), T = (int)txt_qkv.size(1),
              H = (int)txt_qkv.size(3), D = (int)txt_qkv.size(4);
    const int Si = (int)img_qkv.size(1);
    TORCH_CHECK(D % 2 == 0 && D <= 128,
                "pack_joint_qkv: D must be even and <= 128");
    // one set of B, H, D indexes both streams and the joint output
    TORCH_CHECK(txt_qkv.size(2) == 3 && img_qkv.size(2) == 3 &&
                img_qkv.size(0) == B && img_qkv.size(3) == H &&
                img_qkv.size(4) == D,
                "pack_joint_qkv: txt [B,T,3,H,D] and img [B,Si,3,H,D] must "
                "share B, H and D, got txt ", txt_qkv.sizes(), ", img ",
                img_qkv.sizes());
    check_norm_weight("pack_joint_qkv", "wq_t", wq_t, D, txt_qkv);
    check_norm_weight("pack_joint_qkv", "wk_t", wk_t, D, txt_qkv);
    check_norm_weight("pack_joint_qkv", "wq_i", wq_i, D, txt_qkv);
    check_norm_weight("pack_joint_qkv", "wk_i", wk_i, D, txt_qkv);
    check_cs_table("pack_joint_qkv", cs, (long)T + Si, D, txt_qkv);
    TORCH_CHECK(txt_qkv.numel() == 0 || txt_qkv.stride(4) == 1,
                "pack_joint_qkv: txt last dim contiguous");
    TORCH_CHECK(img_qkv.numel() == 0 || img_qkv.stride(4) == 1,
                "pack_joint_qkv: img last dim contiguous");
    auto csf = cs.to(at::kFloat).contiguous();
    auto opts = txt_qkv.options();
    auto oq = at::empty({B, T + Si, H, D}, opts);
    auto ok = at::empty({B, T + Si, H, D}, opts);
    auto ov = at::empty({B, T + Si, H, D}, opts);
    const long rows = (long)B * (T + Si) * H;
    if (rows == 0 || D == 0) return {oq, ok, ov};
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
