// Grouped AdaLN modulation: layer_norm_mod and gate_residual with one
// modulation row per GROUP of consecutive rows. x [B, S, D] dense, modulation
// [B, G, D] with S % G == 0: row s of batch element b takes modulation row
// [b][s / (S / G)]. G = frames is WAN's per-frame timestep, G = S per-token
// modulation, G = 1 the per-batch case in 3-D form. Kernel, then launcher; see
// "Grouped modulation" in docs/KERNELS.md. Needs wave_allreduce_sum
// (token_ops.h) and ln_modulate (norm.h).
//
// Work split, shared by both kernels. The L = S / G rows of one (b, g)
// segment are contiguous in x and share one modulation row. A 256-thread
// block owns a RUN of up to MG_RUN consecutive rows of one segment: the grid
// is segments x ceil(L / MG_RUN), the last run of a segment is short and no
// run crosses a segment edge. The block reads its modulation row once, lane l
// of every wave holding the 16-byte granules l, l + 64, ... (NS slots, so D
// <= 512 * NS) as the packed 16-bit words they were loaded as; wave w then
// takes the rows w, w + 4, ... of the run. There is no LDS and no barrier: a
// wave whose first row lies past the run leaves at once, and the waves of a
// block never wait for each other.
#pragma once

static constexpr int MG_RUN = 16;       // rows per block: four per wave
static constexpr int MG_MAX_D = 8192;   // 16 granules per lane

// Where a block works: its segment's first row plus its run's offset, the
// rows of the run, and the segment's (b, g).
struct MgRun {
    long row0;      // first row of the run, in rows of x
    int rows;       // 1 .. MG_RUN
    long b, g;
};

PA_DEV MgRun mg_run(int G, int L) {
    const int runs = (L + MG_RUN - 1) / MG_RUN;     // per segment
    const long seg = blockIdx.x / runs;             // b * G + g
    const int first = (int)(blockIdx.x % runs) * MG_RUN;
    MgRun r;
    r.row0 = seg * L + first;       // x is dense: segment seg starts at seg * L
    r.rows = min(MG_RUN, L - first);
    r.b = seg / G;
    r.g = seg % G;
    return r;
}

PA_DEV void mg_opaque(short8& v) { asm("" : "+v"(v)); }

// ---------------------------------------------------------------------------
// out = LN(x) * (1 + scale[b][g]) + shift[b][g]. A wave holds its row in
// registers from the one read to the store, so the statistics are the exact
// two-pass ones: the mean, then the sum of the squared deviations, which
// cannot round below zero and keeps its digits on a row at an offset. Both
// reductions are wave_allreduce_sum (DPP and the gfx950 row swaps).
//
// The row stays in the packed 16-bit words it was loaded as and each of the
// three passes decodes it again (one shift for bf16, one convert for fp16).
// Held as fp32 the row takes 8 VGPRs a slot on top of the modulation's 8: at
// D = 5120 (10 slots) that build took 256 VGPRs and 12 AGPRs, one wave a
// SIMD, where this one takes 219 and runs two. mg_opaque keeps the compiler
// from merging the three decodes back into one fp32 copy.
// Slots past DV hold zeros, stay out of the deviations and store nothing; the
// slot loops are unrolled, so no register array is indexed at run time.
// sc_bs / sc_gs (sh_bs / sh_gs): batch and group-row strides of scale (shift)
// in elements.
// ---------------------------------------------------------------------------
template <typename E, int NS>
__global__ __launch_bounds__(256) void layer_norm_mod_grouped_kernel(
    const E* __restrict__ x, const E* __restrict__ scale,
    const E* __restrict__ shift, E* __restrict__ out, int G, int L, int DV,
    long sc_bs, long sc_gs, long sh_bs, long sh_gs, float eps) {
    using EL = Elem16<E>;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x >> 6;
    const MgRun run = mg_run(G, L);
    if (wave >= run.rows) return;
    const short8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const short8* sc = reinterpret_cast<const short8*>(
        scale + run.b * sc_bs + run.g * sc_gs);
    const short8* sh = reinterpret_cast<const short8*>(
        shift + run.b * sh_bs + run.g * sh_gs);

    // the run's modulation row, packed: 8 VGPRs a slot where fp32 (1 + scale)
    // and shift would take 16
    short8 a[NS], c[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int v = lane + i * WAVE;
        a[i] = v < DV ? sc[v] : zero;
        c[i] = v < DV ? sh[v] : zero;
    }

    const float n = (float)(DV * 8);
    for (int r = wave; r < run.rows; r += 4) {
        const long base = (run.row0 + r) * (long)DV;    // in granules
        const short8* xr = reinterpret_cast<const short8*>(x) + base;
        short8 raw[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int v = lane + i * WAVE;
            raw[i] = v < DV ? xr[v] : zero;
        }
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                acc += EL::ld((unsigned short)raw[i][j]);
        }
        const float mean = wave_allreduce_sum(acc) / n;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const bool live = lane + i * WAVE < DV;
            mg_opaque(raw[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d =
                    live ? EL::ld((unsigned short)raw[i][j]) - mean : 0.f;
                sq += d * d;
            }
        }
        const float rstd = rsqrtf(wave_allreduce_sum(sq) / n + eps);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int v = lane + i * WAVE;
            mg_opaque(raw[i]);
            short8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                o[j] = (short)EL::st(ln_modulate<EL>(
                    raw[i][j], a[i][j], c[i][j], mean, rstd));
            if (v < DV) reinterpret_cast<short8*>(out)[base + v] = o;
        }
    }
}

// ---------------------------------------------------------------------------
// out = residual + gate[b][g] * x, the expression of gate_residual_vec_kernel
// in its fp32 order. The gate row stays in registers for the run; the rows
// are streamed through, four slots at a time.
// ---------------------------------------------------------------------------
template <typename E, int NS>
__global__ __launch_bounds__(256) void gate_residual_grouped_kernel(
    const E* __restrict__ res, const E* __restrict__ gate,
    const E* __restrict__ x, E* __restrict__ out, int G, int L, int DV,
    long g_bs, long g_gs) {
    using EL = Elem16<E>;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x >> 6;
    const MgRun run = mg_run(G, L);
    if (wave >= run.rows) return;
    const short8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const short8* gr = reinterpret_cast<const short8*>(
        gate + run.b * g_bs + run.g * g_gs);
    short8 gt[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int v = lane + i * WAVE;
        gt[i] = v < DV ? gr[v] : zero;
    }
    for (int r = wave; r < run.rows; r += 4) {
        const long base = (run.row0 + r) * (long)DV;    // in granules
        const short8* rr = reinterpret_cast<const short8*>(res) + base;
        const short8* xr = reinterpret_cast<const short8*>(x) + base;
        // four slots at a time: their eight loads, then the arithmetic
#pragma unroll
        for (int i0 = 0; i0 < NS; i0 += 4) {
            short8 rv[4], xv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int v = lane + (i0 + k) * WAVE;
                const bool live = i0 + k < NS && v < DV;
                rv[k] = live ? rr[v] : zero;
                xv[k] = live ? xr[v] : zero;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + k >= NS) break;
                const int v = lane + (i0 + k) * WAVE;
                short8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float f = EL::ld((unsigned short)rv[k][j]) +
                              EL::ld((unsigned short)gt[i0 + k][j]) *
                                  EL::ld((unsigned short)xv[k][j]);
                    o[j] = (short)EL::st(f);
                }
                if (v < DV) reinterpret_cast<short8*>(out)[base + v] = o;
            }
        }
    }
}

// A [B, G, D] modulation operand as the grouped kernels read it: rows of D
// contiguous elements that start on 16 bytes, at any batch stride and any
// group-row stride (0 included: an expanded row). The unbind(-2) views of a
// [B, G, 6, D] projection pass as they are; anything else is copied dense.
static at::Tensor mod_group_rows(const at::Tensor& t) {
    const long es = t.element_size();
    const bool ok =
        (t.size(2) <= 1 || t.stride(2) == 1) &&
        (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) == 0 &&
        (t.size(0) <= 1 || (t.stride(0) * es) % 16 == 0) &&
        (t.size(1) <= 1 || (t.stride(1) * es) % 16 == 0);
    return ok ? t : t.contiguous();
}

// x or the residual as the kernels read them: dense, on 16 bytes.
static at::Tensor mod_group_dense(const at::Tensor& t) {
    auto c = t.contiguous();
    return aligned16(c) ? c : c.clone();
}

// The shape rules of both launchers: x [B, S, D] of a 16-bit type with D % 8
// == 0 and D <= MG_MAX_D, `mod` [B, G, D] of x's dtype on x's device with
// G >= 1 dividing S. The kernels index mod[b * bs + g * gs + d] with g < G
// and d < D, and x by rows below B * S: nothing else is read.
static void check_mod_groups(const char* op, const at::Tensor& x,
                             const at::Tensor& mod, const char* name) {
    TORCH_CHECK(x.dim() == 3 && mod.dim() == 3, op, ": x [B, S, D] and ", name,
                " [B, G, D], got ", x.sizes(), " and ", mod.sizes());
    TORCH_CHECK(is_elem16(x.scalar_type()), op, ": bf16 or fp16, got ",
                x.scalar_type());
    const long S = x.size(1), D = x.size(2), G = mod.size(1);
    TORCH_CHECK(D % 8 == 0 && D <= MG_MAX_D, op, ": D % 8 == 0 and D <= ",
                MG_MAX_D, ", got D = ", D);
    TORCH_CHECK(mod.size(0) == x.size(0) && mod.size(2) == D, op, ": ", name,
                " must be [B, G, D] = [", x.size(0), ", G, ", D, "], got ",
                mod.sizes());
    TORCH_CHECK(G >= 1 && S % G == 0, op, ": S = ", S,
                " is not a multiple of G = ", G);
    TORCH_CHECK(mod.scalar_type() == x.scalar_type(), op, ": ", name,
                " dtype (", mod.scalar_type(), ") must match x (",
                x.scalar_type(), ")");
    TORCH_CHECK(mod.device() == x.device(), op, ": ", name, " is on ",
                mod.device(), ", x on ", x.device());
    TORCH_CHECK(x.numel() / std::max<long>(D, 1) <= INT_MAX, op,
                ": too many rows");
}

// Binds NS, the granule slots a lane holds, for DV granules a row.
#define PA_MOD_GROUPS_NS(DV, ...)                                             \
    do {                                                                      \
        if ((DV) <= 64) { constexpr int NS = 1; __VA_ARGS__; }                \
        else if ((DV) <= 128) { constexpr int NS = 2; __VA_ARGS__; }          \
        else if ((DV) <= 256) { constexpr int NS = 4; __VA_ARGS__; }          \
        else if ((DV) <= 384) { constexpr int NS = 6; __VA_ARGS__; }          \
        else if ((DV) <= 512) { constexpr int NS = 8; __VA_ARGS__; }          \
        else if ((DV) <= 640) { constexpr int NS = 10; __VA_ARGS__; }         \
        else if ((DV) <= 768) { constexpr int NS = 12; __VA_ARGS__; }         \
        else { constexpr int NS = 16; __VA_ARGS__; }                          \
    } while (0)

at::Tensor layer_norm_mod_grouped(at::Tensor x, at::Tensor scale,
                                  at::Tensor shift, double eps) {
    CHECK_GPU(x);
    const char* op = "layer_norm_mod_grouped";
    check_mod_groups(op, x, scale, "scale");
    check_mod_groups(op, x, shift, "shift");
    TORCH_CHECK(scale.sizes() == shift.sizes(), op, ": scale ", scale.sizes(),
                " and shift ", shift.sizes(), " must have one shape");
    if (x.numel() == 0) return at::empty(x.sizes(), x.options());
    auto xc = mod_group_dense(x);
    auto out = at::empty_like(xc);
    const int S = (int)xc.size(1), DV = (int)(xc.size(2) / 8);
    const int G = (int)scale.size(1), L = S / G;
    auto sc = mod_group_rows(scale);
    auto sh = mod_group_rows(shift);
    const long blocks = xc.size(0) * G * ((L + MG_RUN - 1) / MG_RUN);
    const auto st = xc.scalar_type();
    PA_MOD_GROUPS_NS(DV, PA_WITH_ELEM16(st, hipLaunchKernelGGL(
        (layer_norm_mod_grouped_kernel<E, NS>), dim3((unsigned)blocks),
        dim3(256), 0, cur_stream(), (const E*)xc.data_ptr(),
        (const E*)sc.data_ptr(), (const E*)sh.data_ptr(),
        (E*)out.data_ptr(), G, L, DV, (long)sc.stride(0), (long)sc.stride(1),
        (long)sh.stride(0), (long)sh.stride(1), (float)eps)));
    return out;
}

at::Tensor gate_residual_grouped(at::Tensor res, at::Tensor gate,
                                 at::Tensor x) {
    CHECK_GPU(x);
    const char* op = "gate_residual_grouped";
    check_mod_groups(op, x, gate, "gate");
    TORCH_CHECK(res.sizes() == x.sizes(), op, ": residual ", res.sizes(),
                " must have x's shape ", x.sizes());
    CHECK_SAME_DEVICE(res, x);
    CHECK_SAME_DTYPE(res, x);
    if (x.numel() == 0) return at::empty(x.sizes(), x.options());
    auto rc = mod_group_dense(res);
    auto xc = mod_group_dense(x);
    auto out = at::empty_like(xc);
    const int S = (int)xc.size(1), DV = (int)(xc.size(2) / 8);
    const int G = (int)gate.size(1), L = S / G;
    auto gc = mod_group_rows(gate);
    const long blocks = xc.size(0) * G * ((L + MG_RUN - 1) / MG_RUN);
    const auto st = xc.scalar_type();
    PA_MOD_GROUPS_NS(DV, PA_WITH_ELEM16(st, hipLaunchKernelGGL(
        (gate_residual_grouped_kernel<E, NS>), dim3((unsigned)blocks),
        dim3(256), 0, cur_stream(), (const E*)rc.data_ptr(),
        (const E*)gc.data_ptr(), (const E*)xc.data_ptr(), (E*)out.data_ptr(),
        G, L, DV, (long)gc.stride(0), (long)gc.stride(1))));
    return out;
}
#undef PA_MOD_GROUPS_NS
