// Exact combination of partial attention results through their log-sum-exp:
// the last step of ring / chunked attention (the LSE instantiations of
// attn_fwd_v4_kernel produce the partials).
#pragma once

#define PA_MERGE_MAX 8  // partials per call: one per GPU of a node

// The N partials' pointers travel by value in the kernel arguments: no
// stacking copy and no pointer table in memory.
struct AttnMergePtrs {
    const void* out[PA_MERGE_MAX];
    const float* lse[PA_MERGE_MAX];
};

// ---------------------------------------------------------------------------
// out_c [rows, D] (16-bit), lse_c [rows] (fp32), c < n. Per row, in fp32:
//   m = max_c lse_c;  m == -inf: out = +0, lse = -inf;  otherwise
//   w_c = exp(lse_c - m), out = (sum_c w_c out_c) / sum_c w_c, rounded once,
//   lse = m + log(sum_c w_c).
// A partial with lse_c == -inf is skipped, never multiplied by 0: its out_c
// is not even loaded, so it is don't-care (NaN included), like a K/V row at
// a masked key. n == 1 reproduces the partial bit for bit (w = 1, x / 1).
//
// One thread per 16-byte vector of a row, D / 8 threads per row, grid-stride.
// The loops over the partials are fully unrolled under the uniform `c < n`,
// so a.out[c] / a.lse[c] are constant kernarg offsets and nothing is indexed
// at run time; all loads of a vector are issued before the first use.
// Bandwidth-bound: (n + 1) * D * 2 + (n + 1) * 4 bytes per row.
// ---------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void attn_merge_kernel(
    AttnMergePtrs a, int n, E* __restrict__ out, float* __restrict__ lse_out,
    long rows, int vecs) {
    using EL = Elem16<E>;
    const long total = rows * vecs;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total;
         idx += (long)gridDim.x * 256) {
        const long row = idx / vecs;
        float l[PA_MERGE_MAX];
        float m = -__builtin_inff();
#pragma unroll
        for (int c = 0; c < PA_MERGE_MAX; ++c) {
            l[c] = -__builtin_inff();
            if (c < n) l[c] = a.lse[c][row];
            m = fmaxf(m, l[c]);
        }
        short8 x[PA_MERGE_MAX];
#pragma unroll
        for (int c = 0; c < PA_MERGE_MAX; ++c) {
            x[c] = short8{0, 0, 0, 0, 0, 0, 0, 0};
            if (c < n && l[c] != -__builtin_inff())
                x[c] = reinterpret_cast<const short8*>(a.out[c])[idx];
        }
        // -0.0 is the exact identity of addition: a partial's -0.0 survives
        float acc[8] = {-0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f};
        float wsum = 0.f;
#pragma unroll
        for (int c = 0; c < PA_MERGE_MAX; ++c) {
            if (c < n && l[c] != -__builtin_inff()) {
                const float w = expf(l[c] - m);
                wsum += w;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    acc[j] = fmaf(w, EL::ld((unsigned short)x[c][j]), acc[j]);
            }
        }
        // m == -inf: no partial saw a key (wsum == 0)
        const bool dead = m == -__builtin_inff();
        short8 y;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            y[j] = (short)EL::st(dead ? 0.f : acc[j] / wsum);
        reinterpret_cast<short8*>(out)[idx] = y;
        if (lse_out != nullptr && idx % vecs == 0)
            lse_out[row] = dead ? m : m + logf(wsum);
    }
}

// outs: n tensors [..., D] of one shape, 16-bit dtype and device, contiguous;
// lses: the n matching fp32 [...] tensors. Returns {out} or {out, lse}.
std::vector<at::Tensor> attn_merge(std::vector<at::Tensor> outs,
                                   std::vector<at::Tensor> lses,
                                   bool return_lse) {
    const int n = (int)outs.size();
    TORCH_CHECK(n >= 1 && n <= PA_MERGE_MAX, "attn_merge: 1 to ",
                PA_MERGE_MAX, " partials, got ", n);
    TORCH_CHECK((int)lses.size() == n, "attn_merge: ", n, " outs but ",
                lses.size(), " lses");
    const at::Tensor& o0 = outs[0];
    CHECK_GPU(o0);
    TORCH_CHECK(is_elem16(o0.scalar_type()),
                "attn_merge: bf16 or fp16 partials only, got ",
                o0.scalar_type());
    TORCH_CHECK(o0.dim() >= 1 && o0.size(-1) > 0 && o0.size(-1) % 8 == 0,
                "attn_merge: the last dim must be a multiple of 8, got ",
                o0.sizes());
    const auto lshape = o0.sizes().slice(0, o0.dim() - 1);
    AttnMergePtrs p;
    for (int c = 0; c < PA_MERGE_MAX; ++c) {
        p.out[c] = nullptr;
        p.lse[c] = nullptr;
    }
    for (int c = 0; c < n; ++c) {
        const at::Tensor& o = outs[c];
        const at::Tensor& l = lses[c];
        TORCH_CHECK(o.device() == o0.device() && l.device() == o0.device(),
                    "attn_merge: partial ", c, " is on ", o.device(),
                    " (lse on ", l.device(), "), partial 0 on ", o0.device());
        TORCH_CHECK(o.scalar_type() == o0.scalar_type(),
                    "attn_merge: partial ", c, " dtype (", o.scalar_type(),
                    ") must match partial 0 (", o0.scalar_type(), ")");
        TORCH_CHECK(l.scalar_type() == at::kFloat,
                    "attn_merge: lse ", c, " must be fp32, got ",
                    l.scalar_type());
        TORCH_CHECK(o.sizes() == o0.sizes(), "attn_merge: partial ", c,
                    " has shape ", o.sizes(), ", partial 0 ", o0.sizes());
        TORCH_CHECK(l.sizes() == lshape, "attn_merge: lse ", c, " has shape ",
                    l.sizes(), ", its partial needs ", lshape);
        TORCH_CHECK(o.is_contiguous() && l.is_contiguous(),
                    "attn_merge: partial ", c, " and its lse must be "
                    "contiguous");
        TORCH_CHECK((reinterpret_cast<uintptr_t>(o.data_ptr()) & 15) == 0,
                    "attn_merge: partial ", c, " is not 16-byte aligned");
        p.out[c] = o.data_ptr();
        p.lse[c] = l.data_ptr<float>();
    }
    at::Tensor out = at::empty_like(o0);
    at::Tensor lse;
    if (return_lse) lse = at::empty_like(lses[0]);
    const int vecs = (int)(o0.size(-1) / 8);
    const long rows = o0.numel() / o0.size(-1);
    if (rows > 0)
        PA_WITH_ELEM16(o0.scalar_type(), hipLaunchKernelGGL(
            HIP_KERNEL_NAME(attn_merge_kernel<E>),
            dim3((unsigned)std::min<long>((rows * vecs + 255) / 256, 16384)),
            dim3(256), 0, cur_stream(), p, n, (E*)out.data_ptr(),
            return_lse ? lse.data_ptr<float>() : nullptr, rows, vecs));
    if (return_lse) return {out, lse};
    return {out};
}
