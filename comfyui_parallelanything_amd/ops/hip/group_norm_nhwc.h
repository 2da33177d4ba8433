// GroupNorm over a dense channels-last tensor x[b][p][c], p < HW: two
// stream-ordered kernels over the same slab decomposition, followed by their
// launcher. Optional affine, SiLU and a per-(batch, channel) addend that is
// applied in fp32 before the statistics: out = GN(x + add).
//
// A slab is npx consecutive pixels of one batch element: npx * C contiguous
// elements, read as 16-byte vectors of 8 channels. With CV = C / 8 vectors
// per pixel, a 256-thread block covers R = 256 / CV pixels per pass (R * CV
// threads active) and thread t keeps column t % CV on every pass, so its
// eight sums and eight sums of squares stay in registers. Beyond 256
// columns (C up to 4096) R = 1 and a thread owns columns t and t + 256
// (NCOL = 2). Channels per group need not divide 8: group membership is per
// channel, taken when the per-thread partials are added up from LDS.
//
//   gn_nhwc_stats_kernel   block (b, slab): per group the slab's (sum, M2),
//                          M2 = sum of squared deviations from the slab's
//                          own mean, into the fp32 workspace [B, S, G, 2]
//   gn_nhwc_apply_kernel   block (b, slab): combines b's S partials per
//                          group in a fixed order (fp64), then streams the
//                          slab
//
// Why (sum, M2) and not (sum, sumsq): sumsq - sum^2 / n loses mean^2 / var
// of the digits it is held in, and an fp32 workspace holds 7. With an
// addend a group can sit at any offset with a variance that comes from the
// addend alone, so the stats kernel adds x and x * x in fp64 (both exact
// for sums of this length: an fp32 value squared has 48 bits), takes M2
// there, and only the centred M2 is rounded to fp32. The apply kernel
// combines slabs around slab 0's mean P, which needs one pass: with d_i =
// mean_i - P, mean = P + sum(n_i d_i) / n and M2 = sum(M2_i) + sum(n_i
// d_i^2) - sum(n_i d_i)^2 / n, where the d_i are small next to P.
//
// No atomics and no inter-block waiting: every sum has one fixed order, so
// results are bitwise reproducible.
#pragma once

static constexpr int GN_THREADS = 256;
static constexpr int GN_MAX_GROUPS = 256;     // one apply-kernel thread each
static constexpr int GN_COL_FLOATS = 2048;    // R * C <= 2048 per NCOL

// Thread geometry shared by the two kernels.
template <int NCOL>
struct GnGeom {
    int CV, R, r, col;
    PA_DEV GnGeom(int C) {
        CV = C / 8;
        if constexpr (NCOL == 1) {
            R = GN_THREADS / CV;
            r = (int)threadIdx.x / CV;      // r >= R: idle thread
            col = (int)threadIdx.x % CV;
        } else {
            R = 1;
            r = 0;
            col = (int)threadIdx.x;         // and col + 256 where < CV
        }
    }
    PA_DEV bool owns(int k) const {
        return NCOL == 1 ? r < R : col + k * GN_THREADS < CV;
    }
};

// The thread's 8 * NCOL addend values in fp32 (zeros without an addend).
template <typename E, int NCOL>
PA_DEV void gn_load_add(const E* add, int b, int C, const GnGeom<NCOL>& g,
                        float (&a)[NCOL][8]) {
    using EL = Elem16<E>;
#pragma unroll
    for (int k = 0; k < NCOL; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[k][j] = 0.f;
        if (add != nullptr && g.owns(k)) {
            const short8 v = *reinterpret_cast<const short8*>(
                add + (long)b * C + (long)(g.col + k * GN_THREADS) * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[k][j] = EL::ld((unsigned short)v[j]);
        }
    }
}

template <typename E, int NCOL>
__global__ __launch_bounds__(GN_THREADS) void gn_nhwc_stats_kernel(
        const E* __restrict__ x, const E* __restrict__ add,
        float* __restrict__ ws, int C, int HW, int G, int npx, int S) {
    using EL = Elem16<E>;
    const int b = blockIdx.x / S, slab = blockIdx.x % S;
    const int p0 = slab * npx, p1 = min(p0 + npx, HW);
    const GnGeom<NCOL> g(C);
    __shared__ double part[NCOL * GN_COL_FLOATS];   // the sums, then the squares

    float a[NCOL][8];
    double s[NCOL][8], q[NCOL][8];
    gn_load_add<E, NCOL>(add, b, C, g, a);
#pragma unroll
    for (int k = 0; k < NCOL; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) s[k][j] = q[k][j] = 0.0;

    const short8* xv = reinterpret_cast<const short8*>(x) + (long)b * HW * g.CV;
#pragma unroll
    for (int k = 0; k < NCOL; ++k) {
        if (!g.owns(k)) continue;
        const int col = g.col + k * GN_THREADS;
#pragma unroll 4
        for (int p = p0 + g.r; p < p1; p += g.R) {
            const short8 v = xv[(long)p * g.CV + col];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // the addend joins in fp32, as in the apply kernel
                const double f =
                    (double)(EL::ld((unsigned short)v[j]) + a[k][j]);
                s[k][j] += f;
                q[k][j] = fma(f, f, q[k][j]);
            }
        }
    }

    // per group, rows then channels in order, first the sums and then,
    // through the same LDS, the squares
    const int cpg = C / G;
    const auto put = [&](const double (&v)[NCOL][8]) {
#pragma unroll
        for (int k = 0; k < NCOL; ++k) {
            if (!g.owns(k)) continue;
            double* d = &part[g.r * C + (g.col + k * GN_THREADS) * 8];
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = v[k][j];
        }
        __syncthreads();
    };
    const auto group_sum = [&](int grp) {
        double t = 0.0;
        for (int r = 0; r < g.R; ++r)
            for (int i = 0; i < cpg; ++i) t += part[r * C + grp * cpg + i];
        return t;
    };
    // G <= 256: thread grp owns group grp
    const int grp = threadIdx.x;
    put(s);
    const double s1 = grp < G ? group_sum(grp) : 0.0;
    __syncthreads();
    put(q);
    if (grp < G) {
        const double s2 = group_sum(grp);
        const double n = (double)(p1 - p0) * (double)cpg;
        float* o = ws + (((long)b * S + slab) * G + grp) * 2;
        o[0] = (float)s1;
        o[1] = (float)fmax(s2 - s1 * s1 / n, 0.0);
    }
}

template <typename E, int NCOL, bool SILU>
__global__ __launch_bounds__(GN_THREADS) void gn_nhwc_apply_kernel(
        const E* __restrict__ x, const E* __restrict__ add,
        const E* __restrict__ w, const E* __restrict__ bias,
        const float* __restrict__ ws, E* __restrict__ out,
        int C, int HW, int G, int npx, int S, float eps) {
    using EL = Elem16<E>;
    const int b = blockIdx.x / S, slab = blockIdx.x % S;
    const int p0 = slab * npx, p1 = min(p0 + npx, HW);
    const GnGeom<NCOL> g(C);
    const int cpg = C / G;
    __shared__ double slabsum[3][GN_THREADS];
    __shared__ float stat[2][GN_MAX_GROUPS];      // mean, rstd

    // the batch element's statistics: thread (k, grp) combines slabs k, k +
    // K, ... of group grp around slab 0's mean P, then thread grp adds the
    // K partial sums in order
    {
        const int K = GN_THREADS / G;
        const int k = (int)threadIdx.x / G, grp = (int)threadIdx.x % G;
        const float* src = ws + ((long)b * S * G + grp) * 2;
        const double P = (double)src[0] / ((double)min(npx, HW) * (double)cpg);
        if (k < K) {
            double A = 0.0, Bq = 0.0, M = 0.0;
            for (int sl = k; sl < S; sl += K) {
                const f32x2 v =
                    *reinterpret_cast<const f32x2*>(src + (long)sl * G * 2);
                const double n_i =
                    (double)(min(sl * npx + npx, HW) - sl * npx) * (double)cpg;
                const double d = (double)v[0] / n_i - P;
                A += n_i * d;
                Bq += n_i * d * d;
                M += (double)v[1];
            }
            slabsum[0][threadIdx.x] = A;
            slabsum[1][threadIdx.x] = Bq;
            slabsum[2][threadIdx.x] = M;
        }
        __syncthreads();
        if ((int)threadIdx.x < G) {
            double A = 0.0, Bq = 0.0, M = 0.0;
            for (int i = 0; i < K; ++i) {
                A += slabsum[0][i * G + threadIdx.x];
                Bq += slabsum[1][i * G + threadIdx.x];
                M += slabsum[2][i * G + threadIdx.x];
            }
            const double inv_n = 1.0 / ((double)cpg * (double)HW);
            stat[0][threadIdx.x] = (float)(P + A * inv_n);
            // clamped for layer_norm_mod_kernel's reason
            stat[1][threadIdx.x] = rsqrtf(
                fmaxf((float)((M + Bq - A * A * inv_n) * inv_n), 0.f) + eps);
        }
        __syncthreads();
    }

    float a[NCOL][8];
    gn_load_add<E, NCOL>(add, b, C, g, a);
    const short8* xv = reinterpret_cast<const short8*>(x) + (long)b * HW * g.CV;
    short8* ov = reinterpret_cast<short8*>(out) + (long)b * HW * g.CV;
#pragma unroll
    for (int k = 0; k < NCOL; ++k) {
        if (!g.owns(k)) continue;
        const int col = g.col + k * GN_THREADS;
        // per channel: the mean stays its own term (not folded into the
        // bias: the folded form loses offset and constant rows)
        float mean[8], sc[8], sh[8];
        short8 wv, bv;
        if (w != nullptr) wv = reinterpret_cast<const short8*>(w)[col];
        if (bias != nullptr) bv = reinterpret_cast<const short8*>(bias)[col];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int grp = (col * 8 + j) / cpg;
            mean[j] = stat[0][grp];
            sc[j] = stat[1][grp];
            if (w != nullptr) sc[j] *= EL::ld((unsigned short)wv[j]);
            sh[j] = bias != nullptr ? EL::ld((unsigned short)bv[j]) : 0.f;
        }
#pragma unroll 4
        for (int p = p0 + g.r; p < p1; p += g.R) {
            const short8 v = xv[(long)p * g.CV + col];
            short8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float f = EL::ld((unsigned short)v[j]) + a[k][j];
                f = (f - mean[j]) * sc[j] + sh[j];
                if constexpr (SILU) f = f / (1.f + __expf(-f));
                o[j] = (short)EL::st(f);
            }
            ov[(long)p * g.CV + col] = o;
        }
    }
}

// x: 4-D dense channels-last, bf16 or fp16, C % 8 == 0, C <= 4096, groups
// <= 256; w, b [C] and add [B, C] of x's dtype on x's device, each
// optional. slab_pixels = 0 picks the slab: at least 16 KiB, and at most
// about 1024 blocks (every apply block reads its batch element's S
// partials, so the workspace traffic grows with S * S).
at::Tensor group_norm_nhwc(at::Tensor x, long groups,
                           std::optional<at::Tensor> w,
                           std::optional<at::Tensor> b,
                           std::optional<at::Tensor> add, double eps,
                           bool silu, long slab_pixels) {
    CHECK_GPU(x);
    TORCH_CHECK(is_elem16(x.scalar_type()),
                "group_norm_nhwc: bf16 or fp16, got ", x.scalar_type());
    TORCH_CHECK(x.dim() == 4 &&
                    x.is_contiguous(at::MemoryFormat::ChannelsLast),
                "group_norm_nhwc expects a dense channels-last [B, C, H, W]");
    const long B = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
    TORCH_CHECK(groups >= 1 && C % groups == 0, "C % groups != 0 (C = ", C,
                ", groups = ", groups, ")");
    TORCH_CHECK(C % 8 == 0, "group_norm_nhwc: C % 8 != 0 (C = ", C, ")");
    TORCH_CHECK(C <= 2 * GN_COL_FLOATS && groups <= GN_MAX_GROUPS,
                "group_norm_nhwc: C <= ", 2 * GN_COL_FLOATS, " and groups <= ",
                GN_MAX_GROUPS, ", got C = ", C, ", groups = ", groups);
    TORCH_CHECK(slab_pixels >= 0, "slab_pixels < 0");
    const void *wp = nullptr, *bp = nullptr, *ap = nullptr;
    if (w.has_value()) {
        const at::Tensor& weight = *w;
        CHECK_GPU(weight);
        CHECK_SAME_DTYPE(weight, x);
        CHECK_SAME_DEVICE(weight, x);
        TORCH_CHECK(weight.dim() == 1 && weight.size(0) == C &&
                        weight.is_contiguous(),
                    "weight must be a contiguous [C] = [", C, "]");
        wp = weight.data_ptr();
    }
    if (b.has_value()) {
        const at::Tensor& bias = *b;
        CHECK_GPU(bias);
        CHECK_SAME_DTYPE(bias, x);
        CHECK_SAME_DEVICE(bias, x);
        TORCH_CHECK(bias.dim() == 1 && bias.size(0) == C &&
                        bias.is_contiguous(),
                    "bias must be a contiguous [C] = [", C, "]");
        bp = bias.data_ptr();
    }
    if (add.has_value()) {
        const at::Tensor& channel_add = *add;
        CHECK_GPU(channel_add);
        CHECK_SAME_DTYPE(channel_add, x);
        CHECK_SAME_DEVICE(channel_add, x);
        TORCH_CHECK(channel_add.dim() == 2 && channel_add.size(0) == B &&
                        channel_add.size(1) == C &&
                        channel_add.is_contiguous(),
                    "channel_add must be a contiguous [B, C] = [", B, ", ", C,
                    "]");
        ap = channel_add.data_ptr();
    }
    // every operand is read as 16-byte vectors
    for (const void* p : {(const void*)x.data_ptr(), wp, bp, ap})
        TORCH_CHECK(((uintptr_t)p & 15) == 0,
                    "group_norm_nhwc: operands must be 16-byte aligned");
    auto out = at::empty_like(x);
    if (x.numel() == 0) return out;
    // the kernels form p0 + npx <= 2 * HW in int
    TORCH_CHECK(HW <= (1L << 30), "group_norm_nhwc: H * W <= 2^30");

    long npx = slab_pixels;
    if (npx == 0)
        npx = std::max((8192 + C - 1) / C, (B * HW + 1023) / 1024);
    npx = std::min(npx, HW);
    const long S = (HW + npx - 1) / npx;
    TORCH_CHECK(B * S < (1L << 31), "group_norm_nhwc: too many slabs");
    auto ws = at::empty({B, S, groups, 2}, x.options().dtype(at::kFloat));

    const dim3 grid((unsigned)(B * S)), block(GN_THREADS);
    const int Ci = (int)C, HWi = (int)HW, G = (int)groups;
    const int npxi = (int)npx, Si = (int)S;
#define GN_LAUNCH(NCOL)                                                       \
    PA_WITH_ELEM16(x.scalar_type(), {                                         \
        hipLaunchKernelGGL((gn_nhwc_stats_kernel<E, NCOL>), grid, block, 0,   \
                           cur_stream(), (const E*)x.data_ptr(),              \
                           (const E*)ap, ws.data_ptr<float>(), Ci, HWi, G,    \
                           npxi, Si);                                         \
        if (silu)                                                             \
            hipLaunchKernelGGL((gn_nhwc_apply_kernel<E, NCOL, true>), grid,   \
                               block, 0, cur_stream(),                        \
                               (const E*)x.data_ptr(), (const E*)ap,          \
                               (const E*)wp, (const E*)bp,                    \
                               ws.data_ptr<float>(), (E*)out.data_ptr(), Ci,  \
                               HWi, G, npxi, Si, (float)eps);                 \
        else                                                                  \
            hipLaunchKernelGGL((gn_nhwc_apply_kernel<E, NCOL, false>), grid,  \
                               block, 0, cur_stream(),                        \
                               (const E*)x.data_ptr(), (const E*)ap,          \
                               (const E*)wp, (const E*)bp,                    \
                               ws.data_ptr<float>(), (E*)out.data_ptr(), Ci,  \
                               HWi, G, npxi, Si, (float)eps);                 \
    })
    if (C / 8 <= GN_THREADS) GN_LAUNCH(1);
    else GN_LAUNCH(2);
#undef GN_LAUNCH
    return out;
}
