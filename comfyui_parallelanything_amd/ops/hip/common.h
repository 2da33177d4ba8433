// Shared by every kernel family: element traits, wave/block reductions and
// the host-side checks and dtype-binding macros. Included first.
#pragma once

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
// Host side: argument checks, current stream, dtype binding.
// ---------------------------------------------------------------------------

#define CHECK_GPU(t) TORCH_CHECK((t).is_cuda(), #t " must be on a HIP device")

// The kernels take raw pointers: every tensor whose pointer is cast to the
// element type of `ref` must carry ref's dtype, or an fp16 buffer would be
// read by a bf16 instantiation (and vice versa).
#define CHECK_SAME_DTYPE(t, ref)                                              \
    TORCH_CHECK((t).scalar_type() == (ref).scalar_type(),                     \
                #t " dtype (", (t).scalar_type(), ") must match " #ref " (",  \
                (ref).scalar_type(), ")")

// ... and live on ref's device: a pointer into another device's (or the
// host's) memory is dereferenced by the kernel as if it were local.
#define CHECK_SAME_DEVICE(t, ref)                                             \
    TORCH_CHECK((t).device() == (ref).device(),                               \
                #t " is on ", (t).device(), ", " #ref " on ", (ref).device())

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

// The scalar rungs: runs the statement(s) with `T` bound to bf16, _Float16
// or float, and raises for any other scalar type. OP names the op in the
// message.
#define PA_WITH_DTYPE(OP, ST, ...)                                            \
    do {                                                                      \
        if ((ST) == at::kBFloat16) { using T = bf16; __VA_ARGS__; }           \
        else if ((ST) == at::kHalf) { using T = _Float16; __VA_ARGS__; }      \
        else if ((ST) == at::kFloat) { using T = float; __VA_ARGS__; }        \
        else TORCH_CHECK(false, OP ": unsupported dtype ", (ST),              \
                         " (bf16, fp16 or fp32)");                            \
    } while (0)

// Blocks of a 256-thread grid-stride launch over n items.
static int grid_1d(long n) {
    return (int)std::min<long>((n + 255) / 256, 4096);
}

// A [B, D] modulation operand (scale, shift, gate) as layer_norm_mod and
// gate_residual read it: rows of D contiguous elements, any row stride.
// `vec` additionally asks for what a 16-byte load needs of the base and of
// the stride. Anything else is copied dense.
static at::Tensor mod_rows(const at::Tensor& t, bool vec) {
    bool ok = t.dim() == 2 && (t.size(1) <= 1 || t.stride(1) == 1);
    if (ok && vec)
        ok = (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) == 0 &&
             (t.size(0) <= 1 || (t.stride(0) * t.element_size()) % 16 == 0);
    return ok ? t : t.contiguous();
}
