// Fused attention forward: key-mask and block-mask packs, the v4 kernel, the
// one launcher and the ten entry points.
#pragma once

using bf16x8 = short8;
#define PA_LOG2E 1.4426950408889634f
#define PA_LN2 0.6931471805599453f

// Half-wave exchange without LDS: combine x with the partner lane's x
// (lane i <-> lane i^32). v_permlane32_swap trades the upper half of its
// first operand for the lower half of its second, so of the two results one
// is this lane's own x and the other its partner's; which is which depends
// on the half, and a commutative f gives both lanes the same bits. A VALU
// op: no ds_bpermute round trip and no lgkmcnt wait in the caller's chain.
template <typename F>
PA_DEV float half_swap_combine(float x, F f) {
    const unsigned int u = __float_as_uint(x);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return f(__uint_as_float((unsigned int)r[0]),
             __uint_as_float((unsigned int)r[1]));
}
// One v_mul_f32 that the SLP vectorizer cannot pair into v_pk_mul_f32
// (packed f32 VALU beside MFMAs costs more than the two scalar ops).
PA_DEV float mul_f32_scalar(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ---------------------------------------------------------------------------
// Key-padding mask pack: [B, Sk] bool (nonzero = attend) -> what the MASKED
// attention instantiations read.
//   words[b][t]  bit j = mask[b][64*t + j]; bits at or beyond Sk are 0
//   live[b][..]  ascending indices of tiles with a nonzero word, compacted
//                to the front (the tail is zero-filled)
//   nlive[b]     how many
// One 256-thread block per batch element (launch-bound, not bandwidth-
// bound): every wave ballots 64 keys per step into the word, then wave 0
// compacts 64 tiles per step with a ballot + prefix popcount. Everything
// stays on the device, so the op is graph-capturable.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_key_mask_kernel(
    const unsigned char* __restrict__ mask, unsigned long long* words,
    int* __restrict__ live, int* __restrict__ nlive, int Sk, int n_tiles) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const unsigned char* mb = mask + (long)b * Sk;
    unsigned long long* wb = words + (long)b * n_tiles;
    int* lb = live + (long)b * n_tiles;
    for (int t = wid; t < n_tiles; t += 4) {
        const int key = t * 64 + lane;
        const bool on = key < Sk && mb[key] != 0;
        const unsigned long long w = __ballot(on);
        if (lane == 0) wb[t] = w;
    }
    __syncthreads();  // words of this batch element visible to wave 0
    if (wid != 0) return;
    int count = 0;
    for (int base = 0; base < n_tiles; base += 64) {
        const int t = base + lane;
        const bool alive = t < n_tiles && wb[t] != 0ull;
        const unsigned long long m = __ballot(alive);
        if (alive)
            lb[count + __popcll(m & ((1ull << lane) - 1ull))] = t;
        count += __popcll(m);
    }
    for (int i = count + lane; i < n_tiles; i += 64) lb[i] = 0;
    if (lane == 0) nlive[b] = count;
}

std::vector<at::Tensor> pack_key_mask(at::Tensor mask) {
    CHECK_GPU(mask);
    TORCH_CHECK(mask.dim() == 2, "pack_key_mask expects a [B, Sk] mask");
    TORCH_CHECK(mask.scalar_type() == at::kBool ||
                    at::isIntegralType(mask.scalar_type(), false),
                "pack_key_mask: bool or integer mask only (nonzero = attend); "
                "additive float biases are not supported, got ",
                mask.scalar_type());
    // integer masks: nonzero -> true, on the device (no host read)
    auto mb = (mask.scalar_type() == at::kBool ? mask : mask.ne(0))
                  .contiguous();
    const int B = (int)mb.size(0), Sk = (int)mb.size(1);
    const int n_tiles = (Sk + 63) / 64;
    auto words = at::empty({B, n_tiles}, mb.options().dtype(at::kLong));
    auto live = at::empty({B, n_tiles}, mb.options().dtype(at::kInt));
    auto nlive = at::empty({B}, mb.options().dtype(at::kInt));
    if (B > 0)
        hipLaunchKernelGGL(pack_key_mask_kernel, dim3((unsigned)B), dim3(256),
                           0, cur_stream(),
                           (const unsigned char*)mb.data_ptr(),
                           (unsigned long long*)words.data_ptr(),
                           live.data_ptr<int>(), nlive.data_ptr<int>(), Sk,
                           n_tiles);
    return {words, live, nlive};
}

// ---------------------------------------------------------------------------
// Block-mask pack: [nq, nk] bool block mask (nonzero = query block qb attends
// key tile t; 256 query rows by 64 keys, shared by batch and heads) plus the
// key-mask words of pack_key_mask_kernel -> one live list per (b, qb), which
// the QLIST attention instantiations read.
//   live[b][qb][..]  ascending tiles t with block[qb][t] != 0 and
//                    words[b][t] != 0, compacted to the front (zero tail)
//   nlive[b][qb]     how many
// A block-live tile whose word is 0 is dropped, so every listed tile holds a
// live key, as the kernel's sentinel arithmetic needs. One wave per (qb, b),
// 64 tiles per step with the ballot + prefix popcount of the key-mask pack's
// wave 0. No host read: graph-capturable behind pack_key_mask_kernel on the
// same stream.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pack_block_lists_kernel(
    const unsigned char* __restrict__ block,
    const unsigned long long* __restrict__ words, int* __restrict__ live,
    int* __restrict__ nlive, int nq, int n_tiles) {
    const int qb = blockIdx.x;
    const int b = blockIdx.y;
    const int lane = threadIdx.x;
    const unsigned char* bm = block + (long)qb * n_tiles;
    const unsigned long long* wb = words + (long)b * n_tiles;
    const long row = (long)b * nq + qb;
    int* lb = live + row * n_tiles;
    int count = 0;
    for (int base = 0; base < n_tiles; base += 64) {
        const int t = base + lane;
        const bool alive = t < n_tiles && bm[t] != 0 && wb[t] != 0ull;
        const unsigned long long m = __ballot(alive);
        if (alive)
            lb[count + __popcll(m & ((1ull << lane) - 1ull))] = t;
        count += __popcll(m);
    }
    for (int i = count + lane; i < n_tiles; i += 64) lb[i] = 0;
    if (lane == 0) nlive[row] = count;
}

// block: [nq, nk] bool/integer; words: [B, nk] from pack_key_mask.
std::vector<at::Tensor> pack_block_lists(at::Tensor block, at::Tensor words) {
    CHECK_GPU(block);
    CHECK_GPU(words);
    TORCH_CHECK(block.dim() == 2,
                "pack_block_lists expects a [nq, nk] block mask");
    TORCH_CHECK(block.scalar_type() == at::kBool ||
                    at::isIntegralType(block.scalar_type(), false),
                "pack_block_lists: bool or integer block mask only (nonzero "
                "= attend); additive float biases are not supported, got ",
                block.scalar_type());
    TORCH_CHECK(words.device() == block.device(),
                "pack_block_lists: words must be on the block mask's device");
    TORCH_CHECK(words.dim() == 2 && words.scalar_type() == at::kLong &&
                    words.is_contiguous(),
                "pack_block_lists: words must be contiguous [B, nk] int64 "
                "(pack_key_mask's)");
    TORCH_CHECK(words.size(1) == block.size(1),
                "pack_block_lists: block mask has ", block.size(1),
                " key tiles, words have ", words.size(1));
    auto bm = (block.scalar_type() == at::kBool ? block : block.ne(0))
                  .contiguous();
    const int nq = (int)bm.size(0), n_tiles = (int)bm.size(1);
    const int B = (int)words.size(0);
    TORCH_CHECK(B <= 65535, "pack_block_lists: batch ", B, " exceeds 65535");
    auto live = at::empty({B, nq, n_tiles}, bm.options().dtype(at::kInt));
    auto nlive = at::empty({B, nq}, bm.options().dtype(at::kInt));
    if (B > 0 && nq > 0)
        hipLaunchKernelGGL(pack_block_lists_kernel,
                           dim3((unsigned)nq, (unsigned)B), dim3(64), 0,
                           cur_stream(), (const unsigned char*)bm.data_ptr(),
                           (const unsigned long long*)words.data_ptr(),
                           live.data_ptr<int>(), nlive.data_ptr<int>(), nq,
                           n_tiles);
    return {live, nlive};
}

// ---------------------------------------------------------------------------
// Attention v4: swapped-QK^T 32x32 structure (guide Appendix B ladder).
//
// mfma_f32_32x32x16_bf16 computing S^T = K·Q^T, so each LANE owns a full
// query ROW: softmax max/sum are a 32-value local reduce + ONE half-wave
// exchange with the partner lane (half_swap_combine, no LDS); running (m, l)
// and the per-tile O-rescale are lane-local scalars. P converts f32->bf16
// in-register
// (v_cvt_pk_bf16_f32) and redistributes across half-waves with
// v_permlane32_swap (T12) — NO P staging through LDS. PV computes
// O^T = V^T · P^T (same P fragments serve as the B operand), keeping the
// output row lane-local for the rescale and the 1/l epilogue.
//
// V operand via gfx950's ds_read_b64_tr_b16 hardware transpose-read (guide
// T10): V is stored ROW-major ([key][dim], plain b128 stores straight from
// the HBM staging registers — no per-element transpose pass) with a
// 40-granule (160-element) row stride, which is ≡ 8 (mod 32) so each
// tr-read cycle hits 32 distinct banks, plus a (key&8)<<1 column XOR that
// keeps the two wave halves bank-disjoint. PV A-fragments are gathered by
// two tr reads per (chunk, tile) from one base VGPR + immediate offsets.
// Gather semantics verified empirically (scripts/tr_probe.hip): within a
// 16-lane group, lane L reg j = element (L&3) of the granule addressed by
// lane (L>>2)+4j. Measured +9.3% flux / +7.4% long-S over the swizzled
// scalar-store image (scripts/attn_ab.hip, within-probe interleaved).
//
// Geometry: 512-thread blocks (8 waves x 32 q-rows = 256 rows/block);
// LDS = K[64][D+8] + row-major V[64][160] = 37.9 KB (D=128) -> two blocks
// co-resident per CU, NOT barrier-synced against each other.
// ---------------------------------------------------------------------------
// The element type E (bf16 or _Float16) enters at three points only: the
// MFMA opcode, the P pack (Elem16<E>::pack2) and the epilogue cast. Every
// LDS layout, tr read and permlane swap is a 16-bit move and is shared;
// the mask sentinel, online-softmax state and accumulators stay fp32.
//
// MASKED (key-padding mask, see pack_key_mask_kernel): the KV loop walks the
// batch element's compacted list of live tiles instead of 0..n_tiles-1, and
// the per-key validity test `key < Sk` becomes that key's bit in the tile's
// 64-bit mask word (bits at or beyond Sk are 0, so the bit implies the
// bound). A dead tile is never loaded or multiplied — the -1e30/-3e30
// sentinel arithmetic relies on every processed tile holding at least one
// live key — and a masked K/V row is staged as zeros, so its contents are
// don't-care. nlive == 0 skips the loop (prologue included) and the
// epilogue's inv_l = 0 writes zeros. Both variants run the same KV loops
// (see "KV loop" in the body); `if constexpr (MASKED)` only picks where the
// trip count, the tile index and the mask word come from, and the unmasked
// instantiations compile to the code they had before the flag existed.
//
// QLIST (block masks, needs MASKED; see pack_block_lists_kernel): the live
// list and its count belong to (batch element, query block) instead of the
// batch element — row b * nq + qtile of live/nlive instead of row b. qtile
// is block-uniform, so everything above holds unchanged; the mask words stay
// per batch element. Nothing else differs from MASKED.
//
// LSE (ring / chunked attention, see attn_merge.h): the epilogue also stores
// the row's natural-log sum over its visible keys of exp(scale * q.k), as
// fp32 ln2 * (m_run + log2(l_run)), and -inf for a row that saw no key
// (l_run == 0). Both half-wave partners hold the row's m_run and l_run, so
// the hi == 0 lane stores, through strides of its own (lse is [B, H, S] or
// [B, S, H]). Nothing before the epilogue differs, and the instantiations
// without the flag compile to the code they had before it existed.
template <int D, typename E, bool MASKED = false, bool QLIST = false,
          bool LSE = false>
__global__ __launch_bounds__(512, 2) void attn_fwd_v4_kernel(
    const E* __restrict__ q, const E* __restrict__ k,
    const E* __restrict__ v, E* __restrict__ out,
    int S, int Sk, float scale, int H,
    long q_bs, long q_hs, int q_ss,
    long k_bs, long k_hs, int k_ss,
    long v_bs, long v_hs, int v_ss,
    long o_bs, long o_hs, int o_ss, int xcd_grid,
    E* __restrict__ out2, int s_split,
    long o2_bs, long o2_hs, int o2_ss,
    const unsigned long long* __restrict__ mask_words = nullptr,
    const int* __restrict__ mask_live = nullptr,
    const int* __restrict__ mask_nlive = nullptr,
    float* __restrict__ lse = nullptr,
    long l_bs = 0, long l_hs = 0, long l_ss = 0) {
    using EL = Elem16<E>;
    constexpr int KVBLK = 64;
    constexpr int WAVES = 8;
    constexpr int THREADS = WAVES * 64;
    constexpr int KPAD = D + 8;
    constexpr int VROW = 160;        // V row stride: 40 granules ≡ 8 mod 32
    constexpr int KK = D / 16;        // QK^T K-steps per 32-key tile
    constexpr int NV = D / 32;        // PV dim tiles
    constexpr int KVECS = (KVBLK * D) / (8 * THREADS);
    // D=128: double-buffered LDS (75.8 KB, still 2 blocks/CU) for the v5a
    // 1-barrier pipelined schedule; D=64 keeps the v4 2-barrier loop.
    constexpr int DBUF = (D == 128) ? 2 : 1;

    __shared__ E k_lds[DBUF * KVBLK * KPAD];
    __shared__ E v_lds[DBUF * KVBLK * VROW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l32 = lane & 31;        // this lane's query row (within wave)
    const int hi = lane >> 5;         // half-wave id
    // tr_b16 per-lane base: this lane supplies the granule
    // (key = hi*8 + (p>>2) [+16c+4rd], col = 32n + 16*((G&1)^hi) + 4*(p&3))
    const int trb = (hi * 8 + ((lane & 15) >> 2)) * VROW +
                    16 * (((lane >> 4) & 1) ^ hi) + 4 * (lane & 3);

    long bh;
    int qtile;
    if (xcd_grid) {
        // XCD-affine decode: xcd = id%8, bh = xcd + 8*(id/8 / nq),
        // qtile = (id/8) % nq  (bijective when BH % 8 == 0)
        const int nq = (S + WAVES * 32 - 1) / (WAVES * 32);
        const long id = blockIdx.x;
        const long xcd = id & 7;
        const long within = id >> 3;
        bh = xcd + 8 * (within / nq);
        qtile = (int)(within % nq);
    } else {
        bh = blockIdx.y;
        qtile = blockIdx.x;
    }
    const long b = bh / H;
    const int h = (int)(bh % H);
    const int q0 = qtile * (WAVES * 32) + wid * 32;

    const E* qp = q + b * q_bs + (long)h * q_hs;
    const E* kp = k + b * k_bs + (long)h * k_hs;
    const E* vp = v + b * v_bs + (long)h * v_hs;
    E* op = out + b * o_bs + (long)h * o_hs;
    E* op2 = out2 ? out2 + b * o2_bs + (long)h * o2_hs : nullptr;

    // Q fragments (B-operand of the swapped QK^T): lane holds
    // Q[q0 + l32][kk*16 + hi*8 + j], j = 0..7.
    bf16x8 qfrag[KK];
    {
        const int row = q0 + l32;
        const int rr = row < S ? row : (S > 0 ? S - 1 : 0);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
            qfrag[kk] = *reinterpret_cast<const bf16x8*>(
                qp + (long)rr * q_ss + kk * 16 + hi * 8);
    }

    f32x16 o_acc[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[n][r] = 0.f;
    float m_run = -1e30f, l_run = 0.f;
    const float scale2 = scale * PA_LOG2E;

    bf16x8 kreg[KVECS], vreg[KVECS];
    // `word` (MASKED only) is the tile's mask word: bit `row` set = stage
    // the row, clear = stage zeros (covers src >= Sk, whose bits are 0)
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
                kreg[i] = *reinterpret_cast<const bf16x8*>(kp + (long)src * k_ss + col);
                vreg[i] = *reinterpret_cast<const bf16x8*>(vp + (long)src * v_ss + col);
            } else {
                kreg[i] = bf16x8{0,0,0,0,0,0,0,0};
                vreg[i] = bf16x8{0,0,0,0,0,0,0,0};
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
            // row-major V, b128 store; column XOR by (row&8)<<1 keeps the
            // tr gather conflict-free under either half-wave pairing
            *reinterpret_cast<bf16x8*>(
                &v_lds[buf * (KVBLK * VROW) + row * VROW +
                       (col ^ ((row & 8) << 1))]) = vreg[i];
        }
    };

    // ---- per-tile phases --------------------------------------------------
    auto qk_phase = [&](int buf, f32x16* st) {
        // swapped QK^T: S^T[key][row] for two 32-key tiles;
        // A = K chunk: lane holds K[kt*32 + l32][kk*16 + hi*8 + j]
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
                st[kt] = EL::mfma32(afrag, qfrag[kk], st[kt]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };
    auto softmax_phase = [&](int kv0, f32x16* st, bf16x8* pfrag,
                             unsigned long long word = 0) {
        // lane-local online softmax (this lane's row = q0 + l32);
        // value (kt, reg) = S[row][key = kt*32 + (reg&3) + 8*(reg>>2) + 4*hi]
        // raw tile max (scale2 > 0 commutes with max), softmax scale fused
        // into the exp2 argument as one FMA per element.
        //
        // Per-key validity only where a tile can hold a dead key: `full` is
        // block-uniform (Sk and kv0 are scalars, the mask word is pinned in
        // SGPRs), so a full tile branches over the whole substitution — no
        // key index, compare or select — and uses the scores as qk_phase
        // left them. Every tile of an Sk % 64 == 0 call is full. The
        // substitution works in place ahead of ONE softmax body: a second,
        // compile-time-full copy of the body costs registers (D=128 spills,
        // D=64 loses a resident block; scripts/attn_v6.hip v4/v5).
        bool full;
        if constexpr (MASKED) full = word == ~0ull;
        else full = kv0 + KVBLK <= Sk;
        if (!full) {
            // MASKED: this lane's keys are bits 4*hi + (r&3) + 8*(r>>2) of
            // the word's half kt — one 64-bit shift, then constant bit
            // positions
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
                    st[kt][r] = valid ? st[kt][r] : -3e30f;
                }
        }
        float mx = -3e30f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[kt][r]);
        // partner: row's other 32 keys
        mx = half_swap_combine(
            mx, [](float a, float c) { return fmaxf(a, c); });
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
        ps = half_swap_combine(ps, [](float a, float c) { return a + c; });
        l_run = l_run * alpha + ps;
        if (alpha != 1.f) {
            // D=128: 64 scalar v_mul_f32; left to the compiler they become
            // 32 v_pk_mul_f32, slower beside the MFMAs there. D=64 measured
            // the other way round and keeps the packed form
            // (scripts/attn_v6.hip, v3 against v2).
#pragma unroll
            for (int n = 0; n < NV; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (D == 128)
                        o_acc[n][r] = mul_f32_scalar(o_acc[n][r], alpha);
                    else
                        o_acc[n][r] *= alpha;
                }
        }
        // P f32 -> 16-bit fragments via cvt_pk + permlane32_swap: chunk c
        // (16 keys) uses regs 8*(c&1)..+7 of st[c>>1]; after the half-swap
        // each lane holds P[row l32][chunk base + hi*8 + j].
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x16& sv = st[c >> 1];
            const int rb = 8 * (c & 1);
            unsigned int w0 = EL::pack2(sv[rb + 0], sv[rb + 1]);
            unsigned int w1 = EL::pack2(sv[rb + 2], sv[rb + 3]);
            unsigned int w2 = EL::pack2(sv[rb + 4], sv[rb + 5]);
            unsigned int w3 = EL::pack2(sv[rb + 6], sv[rb + 7]);
            auto r02 = __builtin_amdgcn_permlane32_swap(w0, w2, false, false);
            auto r13 = __builtin_amdgcn_permlane32_swap(w1, w3, false, false);
            unsigned int d[4] = {(unsigned int)r02[0], (unsigned int)r13[0],
                                 (unsigned int)r02[1], (unsigned int)r13[1]};
            pfrag[c] = *reinterpret_cast<bf16x8*>(d);
        }
    };
    auto pv_phase = [&](int buf, bf16x8* pfrag) {
        // PV: O^T[dim][row] += V^T chunk · P^T chunk; A = V^T gathered from
        // the row-major V image by ds_read_b64_tr_b16 (2 reads per (c, n)).
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int n = 0; n < NV; ++n) {
                short4v alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) short4v*)
                        &v_lds[buf * (KVBLK * VROW) + trb + c * (16 * VROW) +
                               n * 32]);
                short4v ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) short4v*)
                        &v_lds[buf * (KVBLK * VROW) + trb + c * (16 * VROW) +
                               4 * VROW + n * 32]);
                bf16x8 va = __builtin_shufflevector(alo, ahi,
                                                    0, 1, 2, 3, 4, 5, 6, 7);
                o_acc[n] = EL::mfma32(va, pfrag[c], o_acc[n]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };

    // ---- KV loop ----------------------------------------------------------
    // One loop per schedule, written over three block-uniform accessors so
    // the masked and unmasked instantiations share it:
    //   nt          trip count: nlive[b] (MASKED) or n_tiles
    //   tile_at(j)  j-th tile to process: live[b][j] (MASKED) or j
    // (QLIST: read nlive[b][qtile] and live[b][qtile][j] for these two)
    //   word_of(t)  tile t's 64-bit mask word (MASKED) or 0 (ignored)
    // b is uniform across the block, so are nt, every tile index and every
    // mask word: readfirstlane pins them in SGPRs, and trip counts and
    // barriers stay block-uniform. With MASKED, nt == 0 skips the prologue's
    // loads, LDS writes and barrier too; the unmasked prologue is
    // unconditional, as it was before the flag existed.
    const int n_tiles = (Sk + KVBLK - 1) / KVBLK;
    // row of live/nlive: per batch element, or per (b, query block)
    const long lrow =
        QLIST ? b * ((S + WAVES * 32 - 1) / (WAVES * 32)) + qtile : b;
    const int* live_b = MASKED ? mask_live + lrow * n_tiles : nullptr;
    const unsigned long long* words_b =
        MASKED ? mask_words + b * n_tiles : nullptr;
    const int nt =
        MASKED ? __builtin_amdgcn_readfirstlane(mask_nlive[lrow]) : n_tiles;
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
    // (the loads are written out at each site: wrapping tile_at + word_of +
    // issue_tile_loads in one more lambda reorders the unmasked code)
    if constexpr (DBUF == 2) {
        // v5a pipelined schedule (measured +4.0% flux / +4.2% long-S over
        // the 2-barrier loop, scripts/attn_v5.hip): double-buffered LDS,
        // ONE barrier per tile; tile j+1's stores land in the other buffer
        // interleaved where the LDS port is idle (K after QK^T, V after
        // softmax); tile j+2's global loads issue before PV.
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
        for (int j = 0; j < nt; ++j) {
            const int p = j & 1;
            const int tile = tile_at(j);
            f32x16 st[2];
            bf16x8 pfrag[4];
            qk_phase(p, st);
            if (j + 1 < nt) write_k_lds(p ^ 1);
            softmax_phase(tile * KVBLK, st, pfrag, word_of(tile));
            if (j + 1 < nt) write_v_lds(p ^ 1);
            if (j + 2 < nt) {
                const int t2 = tile_at(j + 2);
                issue_tile_loads(t2 * KVBLK, word_of(t2));
            }
            pv_phase(p, pfrag);
            __syncthreads();
        }
    } else {
        // D=64 keeps the v4 2-barrier loop (v5a measured -2.6% there —
        // halved MFMA per tile leaves too little compute to hide stores).
        if (!MASKED || nt > 0) {
            const int t0 = tile_at(0);
            issue_tile_loads(t0 * KVBLK, word_of(t0));
        }
        for (int j = 0; j < nt; ++j) {
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
            softmax_phase(tile * KVBLK, st, pfrag, word_of(tile));
            pv_phase(0, pfrag);
        }
    }

    // ---- epilogue: O = O^T / l, row is lane-local -------------------------
    const int row = q0 + l32;
    if (row < S) {
        // split-stream output: rows >= s_split land in out2 (per-stream
        // contiguous buffers feed the txt/img projections with no reshape
        // copies)
        E* obase;
        long orow;
        int oss;
        if (op2 != nullptr && row >= s_split) {
            obase = op2;
            orow = row - s_split;
            oss = o2_ss;
        } else {
            obase = op;
            orow = row;
            oss = o_ss;
        }
        const float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
        if constexpr (LSE) {
            // m_run is in the log2 domain (scale2 carries log2 e); l_run >= 1
            // once a tile has run, since the running maximum's own key
            // contributes exp2(0)
            if (hi == 0)
                lse[b * l_bs + (long)h * l_hs + (long)row * l_ss] =
                    (l_run > 0.f)
                        ? PA_LN2 * (m_run + __builtin_amdgcn_logf(l_run))
                        : -__builtin_inff();
        }
#pragma unroll
        for (int n = 0; n < NV; ++n) {
#pragma unroll
            for (int r2 = 0; r2 < 4; ++r2) {
                // dims n*32 + 8*r2 + 4*hi + (0..3) are consecutive
                const int dim0 = n * 32 + 8 * r2 + 4 * hi;
                unsigned short pack[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    pack[j] = EL::st(o_acc[n][r2 * 4 + j] * inv_l);
                *reinterpret_cast<unsigned long long*>(
                    obase + orow * oss + dim0) =
                    *reinterpret_cast<unsigned long long*>(pack);
            }
        }
    }
}

// Packed key mask as the MASKED kernels take it (see pack_key_mask). With a
// block mask, live is [B, nq, nk] and nlive [B, nq] (see pack_block_lists),
// which selects the QLIST instantiations.
struct AttnKeyMask {
    at::Tensor words, live, nlive;
};

// Arguments of one attention launch, in the kernel's parameter order.
// Pointers are untyped here; the launch casts them to the element type.
struct AttnArgs {
    const void *q, *k, *v;
    void* out;
    int S, Sk;
    float scale;
    int H;
    long q_bs, q_hs;
    int q_ss;
    long k_bs, k_hs;
    int k_ss;
    long v_bs, v_hs;
    int v_ss;
    long o_bs, o_hs;
    int o_ss, xcd_grid;
    void* out2;
    int s_split;
    long o2_bs, o2_hs;
    int o2_ss;
    const unsigned long long* mask_words;
    const int *mask_live, *mask_nlive;
    float* lse;
    long l_bs, l_hs, l_ss;
};

template <int D, bool MASKED, bool QLIST = false, bool LSE = false>
static void launch_attn_v4(at::ScalarType st, dim3 grid, const AttnArgs& a) {
    PA_WITH_ELEM16(st, hipLaunchKernelGGL(
        HIP_KERNEL_NAME(attn_fwd_v4_kernel<D, E, MASKED, QLIST, LSE>), grid,
        dim3(512), 0,
        cur_stream(), (const E*)a.q, (const E*)a.k, (const E*)a.v, (E*)a.out,
        a.S, a.Sk, a.scale, a.H, a.q_bs, a.q_hs, a.q_ss, a.k_bs, a.k_hs,
        a.k_ss, a.v_bs, a.v_hs, a.v_ss, a.o_bs, a.o_hs, a.o_ss, a.xcd_grid,
        (E*)a.out2, a.s_split, a.o2_bs, a.o2_hs, a.o2_ss, a.mask_words,
        a.mask_live, a.mask_nlive, a.lse, a.l_bs, a.l_hs, a.l_ss));
}

// The one attention launcher. has_split (bshd only) writes rows >= split to
// a second tensor, 0 < split < S; km != nullptr selects the MASKED
// instantiations, and a 3-D km->live their QLIST flavour. want_lse appends
// the fp32 log-sum-exp, in the output's layout without D, to the result; it
// goes with neither a split nor a block mask.
static std::vector<at::Tensor> attn_fwd_launch(
    at::Tensor q, at::Tensor k, at::Tensor v, double scale, bool bshd,
    bool has_split, long split, const AttnKeyMask* km,
    bool want_lse = false) {
    CHECK_GPU(q);
    TORCH_CHECK(is_elem16(q.scalar_type()),
                "attn_fwd: bf16 or fp16 only, got ", q.scalar_type());
    CHECK_SAME_DTYPE(k, q);
    CHECK_SAME_DTYPE(v, q);
    CHECK_SAME_DEVICE(k, q);
    CHECK_SAME_DEVICE(v, q);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4,
                "attn_fwd expects 4-D q/k/v");
    // layouts: bshd = [B, S, H, D] (strided views allowed),
    //          else  = [B, H, S, D] (must be row-contiguous per head)
    const int b_ax = 0, s_ax = bshd ? 1 : 2, h_ax = bshd ? 2 : 1, d_ax = 3;
    const int B = (int)q.size(b_ax), S = (int)q.size(s_ax),
              H = (int)q.size(h_ax), D = (int)q.size(d_ax);
    TORCH_CHECK(D == 64 || D == 128, "attn_fwd: D must be 64 or 128");
    // The kernel indexes k and v with q's batch, head and dim counts: a k
    // or v with fewer of any is read past its end, never broadcast.
    TORCH_CHECK(k.size(b_ax) == B && v.size(b_ax) == B,
                "attn_fwd: k/v batch must equal q's batch (", B, "), got k ",
                k.size(b_ax), ", v ", v.size(b_ax));
    TORCH_CHECK(k.size(h_ax) == H && v.size(h_ax) == H,
                "attn_fwd: k/v heads must equal q's heads (", H, "), got k ",
                k.size(h_ax), ", v ", v.size(h_ax));
    TORCH_CHECK(k.size(d_ax) == D && v.size(d_ax) == D,
                "attn_fwd: k/v head dim must equal q's head dim (", D,
                "), got k ", k.size(d_ax), ", v ", v.size(d_ax));
    TORCH_CHECK(v.size(s_ax) == k.size(s_ax),
                "attn_fwd: v must have k's length (", k.size(s_ax),
                " keys), got ", v.size(s_ax));
    TORCH_CHECK(!want_lse || (!has_split &&
                              (km == nullptr || km->live.dim() != 3)),
                "attn_fwd: the log-sum-exp output goes with neither a split "
                "nor a block mask");
    TORCH_CHECK(!has_split || (split > 0 && split < S),
                "attn_fwd: split must lie inside (0, S = ", S, "), got ",
                split);
    // The kernel's 16-byte vector loads need every stride a multiple of 8
    // elements and a 16-byte aligned base; anything else is copied once.
    auto fix = [&](at::Tensor t) {
        if (t.stride(d_ax) != 1 || (t.stride(s_ax) % 8) != 0 ||
            (t.stride(h_ax) % 8) != 0 || (t.stride(b_ax) % 8) != 0)
            t = t.contiguous();
        if ((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) != 0)
            t = t.clone(at::MemoryFormat::Contiguous);
        return t;
    };
    auto qc = fix(q);
    auto kc = fix(k);
    auto vc = fix(v);
    const int Sk = (int)kc.size(s_ax);
    if (km != nullptr) {
        const long n_tiles = (Sk + 63) / 64;
        TORCH_CHECK(km->words.device() == qc.device() &&
                        km->live.device() == qc.device() &&
                        km->nlive.device() == qc.device(),
                    "attn_fwd: key mask must be on q's device");
        TORCH_CHECK(km->words.scalar_type() == at::kLong &&
                        km->live.scalar_type() == at::kInt &&
                        km->nlive.scalar_type() == at::kInt,
                    "attn_fwd: key mask needs int64 words, int32 live/nlive");
        const bool qlist = km->live.dim() == 3;
        TORCH_CHECK(km->words.dim() == 2 &&
                        (km->live.dim() == 2 || km->live.dim() == 3) &&
                        km->nlive.dim() == km->live.dim() - 1 &&
                        km->words.size(0) == B && km->live.size(0) == B &&
                        km->nlive.size(0) == B,
                    "attn_fwd: key mask batch must equal q's batch (", B, ")");
        TORCH_CHECK(km->words.size(1) == n_tiles &&
                        km->live.size(qlist ? 2 : 1) == n_tiles,
                    "attn_fwd: key mask was packed for another Sk (", Sk,
                    " keys need ", n_tiles, " tiles, got ",
                    km->words.size(1), ")");
        if (qlist) {
            const long nqb = (S + 255) / 256;
            TORCH_CHECK(km->live.size(1) == nqb && km->nlive.size(1) == nqb,
                        "attn_fwd: block mask was packed for another Sq (", S,
                        " rows need ", nqb, " query blocks, got ",
                        km->live.size(1), ")");
        }
        TORCH_CHECK(km->words.is_contiguous() && km->live.is_contiguous() &&
                        km->nlive.is_contiguous(),
                    "attn_fwd: key mask tensors must be contiguous");
    }
    const bool do_split = has_split && bshd;
    at::Tensor out = bshd
        ? at::empty({B, do_split ? (int)split : S, H, D}, qc.options())
        : at::empty({B, H, S, D}, qc.options());
    at::Tensor out2;
    if (do_split) out2 = at::empty({B, S - (int)split, H, D}, qc.options());
    at::Tensor lse;
    if (want_lse)
        lse = bshd ? at::empty({B, S, H}, qc.options().dtype(at::kFloat))
                   : at::empty({B, H, S}, qc.options().dtype(at::kFloat));
    // Nothing to compute: an empty result (a grid of zero blocks is a launch
    // error), or zeros where no row sees a key.
    if (B == 0 || H == 0 || S == 0 || Sk == 0) {
        out.zero_();
        if (want_lse) {
            lse.fill_(-std::numeric_limits<float>::infinity());
            return {out, lse};
        }
        if (do_split) {
            out2.zero_();
            return {out, out2};
        }
        return {out};
    }
    const long BH = (long)B * H;
    const unsigned nq = (unsigned)((S + 255) / 256);
    // 1-D XCD-affine grid: same-(b,h) q-tiles share an XCD's L2
    const bool xcd_grid = BH % 8 == 0;
    const dim3 grid = xcd_grid ? dim3((unsigned)(nq * BH), 1)
                               : dim3(nq, (unsigned)BH);
    const AttnArgs a{
        qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
        S, Sk, (float)scale, H,
        qc.stride(b_ax), qc.stride(h_ax), (int)qc.stride(s_ax),
        kc.stride(b_ax), kc.stride(h_ax), (int)kc.stride(s_ax),
        vc.stride(b_ax), vc.stride(h_ax), (int)vc.stride(s_ax),
        out.stride(b_ax), out.stride(h_ax), (int)out.stride(s_ax),
        xcd_grid ? 1 : 0,
        do_split ? out2.data_ptr() : nullptr, do_split ? (int)split : S,
        do_split ? out2.stride(0) : 0, do_split ? out2.stride(2) : 0,
        do_split ? (int)out2.stride(1) : 0,
        km ? (const unsigned long long*)km->words.data_ptr() : nullptr,
        km ? km->live.data_ptr<int>() : nullptr,
        km ? km->nlive.data_ptr<int>() : nullptr,
        want_lse ? lse.data_ptr<float>() : nullptr,
        want_lse ? lse.stride(b_ax) : 0, want_lse ? lse.stride(h_ax) : 0,
        want_lse ? lse.stride(s_ax) : 0};
    const at::ScalarType st = qc.scalar_type();
    if (want_lse) {
        if (km != nullptr) {
            if (D == 128) launch_attn_v4<128, true, false, true>(st, grid, a);
            else launch_attn_v4<64, true, false, true>(st, grid, a);
        } else {
            if (D == 128) launch_attn_v4<128, false, false, true>(st, grid, a);
            else launch_attn_v4<64, false, false, true>(st, grid, a);
        }
        return {out, lse};
    }
    if (km != nullptr && km->live.dim() == 3) {
        if (D == 128) launch_attn_v4<128, true, true>(st, grid, a);
        else launch_attn_v4<64, true, true>(st, grid, a);
    } else if (km != nullptr) {
        if (D == 128) launch_attn_v4<128, true>(st, grid, a);
        else launch_attn_v4<64, true>(st, grid, a);
    } else {
        if (D == 128) launch_attn_v4<128, false>(st, grid, a);
        else launch_attn_v4<64, false>(st, grid, a);
    }
    if (do_split) return {out, out2};
    return {out};
}

at::Tensor attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v, double scale) {
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/false, false, 0,
                           nullptr)[0];
}

at::Tensor attn_fwd_bshd(at::Tensor q, at::Tensor k, at::Tensor v, double scale) {
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, false, 0,
                           nullptr)[0];
}

std::vector<at::Tensor> attn_fwd_bshd_split(at::Tensor q, at::Tensor k,
                                            at::Tensor v, double scale,
                                            long split) {
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, true, split,
                           nullptr);
}

at::Tensor attn_fwd_masked(at::Tensor q, at::Tensor k, at::Tensor v,
                           double scale, at::Tensor words, at::Tensor live,
                           at::Tensor nlive) {
    const AttnKeyMask km{words, live, nlive};
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/false, false, 0,
                           &km)[0];
}

at::Tensor attn_fwd_bshd_masked(at::Tensor q, at::Tensor k, at::Tensor v,
                                double scale, at::Tensor words,
                                at::Tensor live, at::Tensor nlive) {
    const AttnKeyMask km{words, live, nlive};
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, false, 0,
                           &km)[0];
}

std::vector<at::Tensor> attn_fwd_bshd_split_masked(
    at::Tensor q, at::Tensor k, at::Tensor v, double scale, long split,
    at::Tensor words, at::Tensor live, at::Tensor nlive) {
    const AttnKeyMask km{words, live, nlive};
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, true, split, &km);
}

std::vector<at::Tensor> attn_fwd_lse(at::Tensor q, at::Tensor k, at::Tensor v,
                                     double scale) {
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/false, false, 0, nullptr,
                           /*want_lse=*/true);
}

std::vector<at::Tensor> attn_fwd_bshd_lse(at::Tensor q, at::Tensor k,
                                          at::Tensor v, double scale) {
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, false, 0, nullptr,
                           /*want_lse=*/true);
}

std::vector<at::Tensor> attn_fwd_lse_masked(at::Tensor q, at::Tensor k,
                                            at::Tensor v, double scale,
                                            at::Tensor words, at::Tensor live,
                                            at::Tensor nlive) {
    const AttnKeyMask km{words, live, nlive};
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/false, false, 0, &km,
                           /*want_lse=*/true);
}

std::vector<at::Tensor> attn_fwd_bshd_lse_masked(
    at::Tensor q, at::Tensor k, at::Tensor v, double scale, at::Tensor words,
    at::Tensor live, at::Tensor nlive) {
    const AttnKeyMask km{words, live, nlive};
    return attn_fwd_launch(q, k, v, scale, /*bshd=*/true, false, 0, &km,
                           /*want_lse=*/true);
}
