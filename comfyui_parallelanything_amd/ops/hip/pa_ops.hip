// MI355X (gfx950, CDNA4) native kernels for comfyui_parallelanything_amd.
//
// Hand-written HIP: fused attention (MFMA 32x32x16 bf16/fp16, LDS-tiled),
// AdaLN-modulated LayerNorm, RMSNorm, GroupNorm+SiLU (NCHW) and GroupNorm
// (channels-last), RoPE apply, gated
// residual, timestep embedding. No CUDA-compat shims, no hipify: the code
// targets gfx950 only (wave64, 4xSIMD-32 CUs, 160 KiB LDS, per-XCD L2).
//
// One translation unit: this file is the includes plus the pybind table.
// The kernels live in the headers beside it, one per kernel family, each
// kernel followed by its launcher, included in dependency order (see
// "Source layout" in docs/KERNELS.md).
//
// These replace the per-step model math the reference node left to stock
// PyTorch inside ComfyUI's model implementations: the
// reference repo has no native code, so every kernel here is new work
// driven by the behavioral contract of the ops/reference.py functions,
// which are the fp32 ground truth in tests/test_gpu_kernels.py.
//
// Build: ops/build.py (hipcc --offload-arch=gfx950, in-tree .so).

#include "common.h"
#include "norm.h"
#include "group_norm_nhwc.h"
#include "elementwise.h"
#include "qk_pack.h"
#include "fp8.h"
#include "attention.h"
#include "attn_merge.h"

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
    m.def("group_norm_nhwc", &group_norm_nhwc,
          "GroupNorm [+ SiLU] of a channels-last tensor, optional per-(b, c) "
          "addend before the statistics (gfx950)",
          py::arg("x"), py::arg("groups"), py::arg("weight") = py::none(),
          py::arg("bias") = py::none(), py::arg("channel_add") = py::none(),
          py::arg("eps") = 1e-6, py::arg("silu") = false,
          py::arg("slab_pixels") = 0);
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
    m.def("pack_block_lists", &pack_block_lists,
          "[nq,nk] block mask + key-mask words -> per-(b, q-block) live "
          "tile lists [B,nq,nk] and counts [B,nq]");
    m.def("attn_fwd_masked", &attn_fwd_masked,
          "attn_fwd with a packed key-padding mask (dead tiles skipped)");
    m.def("attn_fwd_bshd_masked", &attn_fwd_bshd_masked,
          "attn_fwd_bshd with a packed key-padding mask");
    m.def("attn_fwd_bshd_split_masked", &attn_fwd_bshd_split_masked,
          "attn_fwd_bshd_split with a packed key-padding mask");
    m.def("attn_fwd_lse", &attn_fwd_lse,
          "attn_fwd returning (out, fp32 log-sum-exp [B,H,S])");
    m.def("attn_fwd_bshd_lse", &attn_fwd_bshd_lse,
          "attn_fwd_bshd returning (out, fp32 log-sum-exp [B,S,H])");
    m.def("attn_fwd_lse_masked", &attn_fwd_lse_masked,
          "attn_fwd_lse with a packed key-padding mask");
    m.def("attn_fwd_bshd_lse_masked", &attn_fwd_bshd_lse_masked,
          "attn_fwd_bshd_lse with a packed key-padding mask");
    m.def("attn_merge", &attn_merge,
          "Merge up to 8 partial attention results through their "
          "log-sum-exp (gfx950)",
          py::arg("outs"), py::arg("lses"), py::arg("return_lse") = false);
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
