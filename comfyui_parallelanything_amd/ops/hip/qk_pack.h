// Fused qk RMSNorm + RoPE (in place) and the dual-stream joint qkv pack:
// argument checks and launchers. The kernels are in qk_pack_kernels.h.
#pragma once

#include "qk_pack_kernels.h"

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

// Eligibility of the token-major kernels (qk_pack_kernels.h).
static bool ptr16(const at::Tensor& t) {
    return (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) == 0;
}

// A [.., S, H, D] view of 16-bit elements whose heads are contiguous per
// token and whose base and outer strides (dims 0 .. token dim) allow
// 16-byte accesses. `tok_dim` is the index of S; dim `h_dim` is H.
static bool tok_major(const at::Tensor& t, int tok_dim, int h_dim, long D) {
    if (!ptr16(t)) return false;
    if (t.size(h_dim) > 1 && t.stride(h_dim) != D) return false;
    for (int d = 0; d <= tok_dim; ++d)
        if (t.size(d) > 1 && (t.stride(d) % 8) != 0) return false;
    return true;
}

// Wave instructions (512 elements each) of one token that a wave walks.
// Measured at the flagship's H * D = 3072 among 2, 3 and 6 (docs/KERNELS.md,
// "Bandwidth tail"): 2 is the fastest for qk_norm_rope_ in every round and
// ties 3 for the pack.
static constexpr int QK_TOK_CH = 2;

// (chunks per token, waves) of a token-major launch, or nchunk = 0 when the
// 32-bit index arithmetic of the kernels would not hold it.
static std::pair<unsigned, unsigned> tok_work(long tokens, long HD) {
    const long nchunk = (HD + QK_TOK_CH * 512 - 1) / (QK_TOK_CH * 512);
    const long waves = tokens * nchunk;
    if (HD >= (1L << 30) || waves >= (1L << 31) - 4) return {0u, 0u};
    return {(unsigned)nchunk, (unsigned)waves};
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
    const auto work = tok_work((long)B * S, (long)H * D);
    if ((D == 128 || D == 64) && work.first != 0 && tok_major(q, 1, 2, D) &&
        tok_major(k, 1, 2, D) && ptr16(csf) && ptr16(wqc) && ptr16(wkc)) {
#define PA_QK_TOK(DT)                                                         \
        PA_WITH_ELEM16(q.scalar_type(), hipLaunchKernelGGL(                   \
            (qk_norm_rope_tok_kernel<E, DT, QK_TOK_CH, true>),                \
            dim3((work.second + 3) / 4), dim3(256), 0, cur_stream(),          \
            (E*)q.data_ptr(), (E*)k.data_ptr(), (const E*)wqc.data_ptr(),     \
            (const E*)wkc.data_ptr(), csf.data_ptr<float>(), (unsigned)S,     \
            H * D, D, q.stride(0), q.stride(1), k.stride(0), k.stride(1),     \
            work.first, work.second, (float)eps))
        if (D == 128) PA_QK_TOK(128); else PA_QK_TOK(64);
#undef PA_QK_TOK
        return;
    }
    const long blocks = (((rows + 3) / 4) * 64 + 255) / 256;
    PA_WITH_ELEM16(q.scalar_type(), hipLaunchKernelGGL(
        qk_norm_rope_kernel<E>, dim3((unsigned)blocks), dim3(256), 0,
        cur_stream(), (E*)q.data_ptr(), (E*)k.data_ptr(),
        (const E*)wqc.data_ptr(), (const E*)wkc.data_ptr(),
        csf.data_ptr<float>(), S, H, D,
        q.stride(0), q.stride(2), q.stride(1),
        k.stride(0), k.stride(2), k.stride(1), rows, (float)eps));
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
    auto wqtc = wq_t.contiguous(), wktc = wk_t.contiguous();
    auto wqic = wq_i.contiguous(), wkic = wk_i.contiguous();
    const auto work = tok_work((long)B * (T + Si), (long)H * D);
    // a stream of no tokens is never read; dim 2 (q/k/v) is an outer stride
    const bool t_ok = T == 0 || tok_major(txt_qkv, 2, 3, D);
    const bool i_ok = Si == 0 || tok_major(img_qkv, 2, 3, D);
    if ((D == 128 || D == 64) && work.first != 0 && t_ok && i_ok &&
        ptr16(csf) && ptr16(wqtc) && ptr16(wktc) && ptr16(wqic) &&
        ptr16(wkic) && ptr16(oq) && ptr16(ok) && ptr16(ov)) {
#define PA_PACK_TOK(DT)                                                       \
        PA_WITH_ELEM16(txt_qkv.scalar_type(), hipLaunchKernelGGL(             \
            (pack_joint_qkv_tok_kernel<E, DT, QK_TOK_CH, true>),              \
            dim3((work.second + 3) / 4), dim3(256), 0, cur_stream(),          \
            (const E*)txt_qkv.data_ptr(), (const E*)img_qkv.data_ptr(),       \
            (const E*)wqtc.data_ptr(), (const E*)wktc.data_ptr(),             \
            (const E*)wqic.data_ptr(), (const E*)wkic.data_ptr(),             \
            csf.data_ptr<float>(), (E*)oq.data_ptr(), (E*)ok.data_ptr(),      \
            (E*)ov.data_ptr(), (unsigned)T, (unsigned)(T + Si), H * D, D,     \
            txt_qkv.stride(0), txt_qkv.stride(1), txt_qkv.stride(2),          \
            img_qkv.stride(0), img_qkv.stride(1), img_qkv.stride(2),          \
            work.first, work.second, (float)eps))
        if (D == 128) PA_PACK_TOK(128); else PA_PACK_TOK(64);
#undef PA_PACK_TOK
        return {oq, ok, ov};
    }
    const long blocks = (((rows + 3) / 4) * 64 + 255) / 256;
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
