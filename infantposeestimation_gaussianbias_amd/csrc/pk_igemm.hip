// Implicit-GEMM on MFMA (bf16 in, fp32 accumulate) for every dense contraction of the network:
//   3x3 / 1x1 convolutions (forward, and data-gradient as a convolution with flipped weights), and linear layers
//   with an optional row gather/scatter (window partition / reverse of the HRFormer blocks).
//
//   out[m][n] = sum_{t < T} sum_{c < Cin}  A(m, t, c) * Wt[n][t][c]          m < M, n < N
//     conv   : m = (b,oy,ox), t = (kh,kw), A = X[b][oy*s+kh-p][ox*s+kw-p][c] (0 outside; NHWC)
//     dilated: A = X[b][(oy+kh-p)/2][(ox+kw-p)/2][c] only where both numerators are even (stride-2 dgrad)
//     linear : T = 1, A = X[rowmap ? rowmap[m] : m][c]   (rowmap -1 -> zero row: the reference's zero pad tokens)
//
// Tiling (one 256-thread workgroup = 4 waves): BM=128 output rows x BN (32/64/128) output columns, K-step 32
// (one MFMA k), per filter tap.  Operands are staged global -> registers -> LDS (double-buffered, one barrier per
// K-step, rows padded to 80 B against bank conflicts); fragments are read with 16-byte ds_read and fed to
// v_mfma_f32_16x16x32_bf16 with the WEIGHT tile as the A operand, so a lane's 4 accumulator registers are 4
// consecutive output channels of one pixel -> one 8-byte NHWC store per tile per lane.
//
// Epilogue options: bias, exact-erf GELU, residual add with a per-sample scale (DropPath), row scatter, bf16 or
// fp32 output, NCHW-planar fp32 output (head), softplus, and per-tile column sums / sums of squares of the fp32
// accumulators (train-mode BatchNorm statistics, reduced later in fixed order -> deterministic).
//
// This unit holds the forward and data-gradient family: k_igemm2 (the general tile kernel) and its grouped form k_igemm2g, k_conv8p (ring
// kernel of the head convs), k_conv3h (halo kernel of the small-channel 3x3 convs), the routing function that picks among them
// (igemm_route) and the entry points pk_conv2d_nhwc, pk_conv2d_affine_nhwc, pk_conv2d_group, pk_conv_stats_rows and pk_linear_bf16.
// The weight gradients of the same layers are in pk_wgrad.hip.
#include "pk_common.h"

#define STAT_ROWS 128      // pixel rows per BatchNorm partial-statistics tile (pk_conv_stats_tiles)
#define BKK 32
#define LDS_PITCH 40  // bf16 elements per LDS row (32 + 8 pad) = 80 bytes, keeps 16-byte alignment

struct IgemmArgs {
    const uint16_t* x;        // activations, bf16 NHWC [B][Hs][Ws][Cin] or [rows][Cin]
    const uint16_t* w;        // weights bf16 [N][T][Cin]
    void* out;                // see out_mode
    const float* bias;        // [N] or null
    const float* col_scale;   // [N] or null: the accumulator is multiplied by it before the bias (eval-mode BatchNorm folded into the conv)
    const uint16_t* res;      // residual, same layout as a bf16 row-major output, or null
    const float* res_scale;   // per-sample multiplier of the GEMM result before the residual add, [B] or null
    const int32_t* a_rowmap;  // [M] source row or -1 (linear mode only), or null
    const int32_t* o_rowmap;  // [M] destination row or -1 (skip), or null
    float* stats;             // [gridDim.x][2][N] per-M-tile column sums / sums of squares, or null
    uint16_t* preact;         // optional bf16 row-major copy of (acc + bias) BEFORE the activation (saved for GELU backward)
    const uint16_t* gelu_of;  // optional bf16 row-major z: result is multiplied by gelu'(z) (backward through GELU)
    int M, N, Cin, T;         // T = 1 or 9
    int Hs, Ws;               // source spatial size (conv)
    int Ho, Wo;               // output spatial size (conv)
    int stride, pad, dilated; // conv geometry
    int ldo;                  // output row pitch in elements (row-major modes)
    int rows_per_sample;      // rows of one sample (for res_scale): Ho*Wo or tokens per image
    int act;                  // 0 none, 1 GELU(erf), 2 softplus, 3 ReLU applied AFTER the residual add
    int out_mode;             // 0 bf16 row-major, 1 fp32 row-major, 2 fp32 NCHW planes [B][N][Ho*Wo]
    int xcd_remap;            // set by igemm_launch: XCD-contiguous tile order
    int vec8;                 // set by igemm_launch: row-major pointers 16-byte aligned and ldo % 8 == 0 -> 16-byte epilogue I/O
    int chunk_major;          // set by igemm_launch: K order = all taps of one channel chunk back to back (N <= 32 tiles of deep 3x3 convs)
    int dil_group;            // set by igemm_launch (stride-2 data gradients): output pixels enumerated parity class by parity class
};

// ================================================================================================ main kernel (k_igemm2)
// The contraction and epilogue of the header comment, arranged so that the K loop is MFMA-bound instead of issue-bound:
//   * filter taps are the OUTER loop: per tap each thread computes ONE byte offset per staged row (bounds, dilation);
//     the inner loop over channel chunks only bumps a scalar offset;
//   * every global read is a branch-free `buffer_load_dwordx4`: an out-of-image tap, a row beyond M, a pad token or a
//     channel beyond Cin gets the offset 0x80000000 >= num_records and the hardware returns zeros;
//   * LDS tiles are unpadded and XOR-swizzled per 16-byte chunk (conflict-free ds_read_b128 for both K-steps:
//     BK=64: chunk ^= (row>>1)&7, BK=32: chunk ^= (row>>3)<<1, found by exhaustive search over the b128 lane groups).
template <int BK>
__device__ __forceinline__ int swz(int row) { return BK == 64 ? ((row >> 1) & 7) : (((row >> 3) & 1) << 1); }
// floor(q / d) for 0 <= q < 2^24 (d >= 1): float estimate + one correction, ~8 VALU (a 32-bit integer division by a run-time divisor
// compiles to ~35; the pixel decompositions of the output-bound conv launches spent more issue slots on them than on MFMAs)
__device__ __forceinline__ int fast_div24(int q, int d, float inv) {
    int r = (int)((float)q * inv);
    const int rem = q - r * d;
    r += rem >= d ? 1 : (rem < 0 ? -1 : 0);
    return r;
}

// Epilogue of ONE output row segment: this lane owns output row `orow` (pixel / token) and the 8 consecutive columns
// n..n+7, handed over as two float4 read back from the LDS staging tile.  The accumulators are staged through LDS so
// that (a) every global access of the epilogue is a 16-byte access and a wave covers whole 128/256-byte row segments
// (the MFMA C layout would give 8-byte pieces of 16 different rows per instruction), and (b) the epilogue is ONE rolled
// loop: unrolled per accumulator tile it was ~2000 instructions x 16 tiles (erff inlined 64 times, 250 KB of code for
// one kernel), which made the K=32 GEMMs instruction-fetch bound.  Only static indexing of v[] (no scratch).
__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

__device__ __forceinline__ void igemm_epilogue_row8(const IgemmArgs& p, f32x4 lo, f32x4 hi, f32x4 slo, f32x4 shi, f32x4 blo, f32x4 bhi, int orow, int n,
                                                    float rs, int hw_out) {
    if (p.col_scale) {                                    // per-column scale of this lane's 8 columns, then the bias (zeros when absent)
        lo = lo * slo + blo;
        hi = hi * shi + bhi;
    } else {
        lo += blo;
        hi += bhi;
    }
    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    const int nv = p.N - n;                               // valid columns of this segment (>= 1)
    const bool vec = p.vec8 && nv >= 8;
    const size_t base = (size_t)orow * p.ldo + n;
    if (p.preact) {
        if (vec) {
            *reinterpret_cast<u32x4*>(p.preact + base) =
                (u32x4){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nv) p.preact[base + j] = f32_to_bf16(v[j]);
        }
    }
    if (p.gelu_of) {
        if (vec) {
            const u32x4 zz = *reinterpret_cast<const u32x4*>(p.gelu_of + base);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[2 * j] *= gelu_grad(bf16_lo(zz[j]));
                v[2 * j + 1] *= gelu_grad(bf16_hi(zz[j]));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nv) v[j] *= gelu_grad(bf16_to_f32(p.gelu_of[base + j]));
        }
    }
    if (p.act == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gelu_erf(v[j]);
    } else if (p.act == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = softplus_(v[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= rs;
    if (p.out_mode == 2) {
        const int bb = orow / hw_out, pix = orow - bb * hw_out;
        float* o = reinterpret_cast<float*>(p.out) + ((size_t)bb * p.N + n) * hw_out + pix;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < nv) o[(size_t)j * hw_out] = v[j];
        return;
    }
    if (p.res) {
        if (vec) {
            const u32x4 rv = *reinterpret_cast<const u32x4*>(p.res + base);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[2 * j] += bf16_lo(rv[j]);
                v[2 * j + 1] += bf16_hi(rv[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nv) v[j] += bf16_to_f32(p.res[base + j]);
        }
    }
    if (p.act == 3) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    if (p.out_mode == 0) {
        uint16_t* o = reinterpret_cast<uint16_t*>(p.out) + base;
        if (vec) {
            *reinterpret_cast<u32x4*>(o) =
                (u32x4){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nv) o[j] = f32_to_bf16(v[j]);
        }
    } else {
        float* o = reinterpret_cast<float*>(p.out) + base;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nv) o[j] = v[j];
        }
    }
}

// Every instantiation is one of four specialisations (LEAN = 1 .. 4; there is no kernel with every run-time mode left in):
//   1: the token GEMMs of the HRFormer blocks only (linear rows with optional gather / scatter maps, bias, residual with a per-sample
//      scale, bf16 output) -- the convolution addressing, the activations, the fp32 / NCHW outputs and the statistics are compiled out.  The
//      full kernel is 27-30 KB of code; a small launch (100-900 workgroups, 1-4 K-steps) spends much of its few microseconds fetching it cold.
//   2: as 1, with the GELU epilogues kept;  3: every epilogue, plain addressing;  4: every epilogue, dilated gather (see the first lines).
// The kernel body takes its tile coordinates and grid shape as arguments: k_igemm2 passes blockIdx / gridDim, the GROUPED launch
// k_igemm2g (below) cuts one 1-D grid into the tile grids of several independent problems.
template <int BM, int BN, int WM, int WN, int BK, int LEAN>
__device__ __forceinline__ void igemm2_body(const IgemmArgs& p_in, const int bid_x, const int bid_y, const int grid_x, const int grid_y) {
    static_assert(LEAN >= 1 && LEAN <= 4, "igemm2_body: LEAN is 1, 2, 3 or 4");
    IgemmArgs p = p_in;
    if (LEAN == 3) {
        // every feature of the epilogue, but the PLAIN addressing in the K loop: no dilated gather (stride-2 data gradients), no parity
        // grouping, no chunk-major order.  The generic loop body is 681 instructions around 8 MFMAs on the 128 x 32 tile (295 VALU, 360 SALU,
        // 52 branches: the run-time flags of those three modes are tested in every advance / set_tap) -- ~0.8 us per K-step whatever the
        // tile does, which is what bounds the deep contractions of the low-resolution branches.  With the flags constant the compiler drops it.
        p.dilated = 0; p.dil_group = 0;       // (chunk-major stays a run-time flag of the 128 x 32 tiles: with the mask form a tap change per step is cheap)
    } else if (LEAN == 4) {          // the stride-2 data gradients (dilated gather, grouped or not): no chunk-major order
        p.dilated = 1; p.chunk_major = 0;
    } else {                         // LEAN = 2 keeps the GELU epilogues (fc1: GELU + saved pre-activation; fc2 data gradient: x gelu'(z))
        p.stats = nullptr;
        p.out_mode = 0; p.T = 1; p.Ho = 0; p.Wo = 0; p.dilated = 0; p.vec8 = 1; p.chunk_major = 0; p.dil_group = 0;
        p.col_scale = nullptr;
        if (LEAN == 1) { p.preact = nullptr; p.gelu_of = nullptr; p.act = 0; }
        else if (p.act != 1) p.act = 0;
    }
    constexpr int MI = BM / WM / 16, NI = BN / WN / 16;
    constexpr int CH = BK / 8;                       // 16-byte chunks per tile row
    constexpr int A_PT = BM * CH / 256;              // A chunks per thread (2 or 4)
    constexpr int B_PT = (BN * CH + 255) / 256;      // B chunks per thread (1..4)
    constexpr int KS = BK / 32;                      // MFMA k-steps per staged tile
    constexpr int TM = BM / WM, TN = BN / WN;        // tile of one wave
    constexpr int EP = TN + 4;                       // fp32 pitch of the epilogue staging tile (conflict-free b128 rows)
    constexpr int BPP = (MI > 4) ? 2 : MI;           // 16-row accumulator blocks staged per epilogue pass (all of them for BM = 128)
    constexpr int MAIN_HALFS = 2 * BM * BK + 2 * BN * BK, EPI_HALFS = 4 * (BPP * 16) * EP * 2;
    __shared__ __attribute__((aligned(16))) uint16_t smem[MAIN_HALFS > EPI_HALFS ? MAIN_HALFS : EPI_HALFS];
    uint16_t* sA = smem;                             // [2][BM*BK]
    uint16_t* sB = smem + 2 * BM * BK;               // [2][BN*BK]
    float* sStat = reinterpret_cast<float*>(smem);   // [WM][BN][2], reused after the main loop

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    // XCD-aware tile order.  Workgroups are handed to the 8 XCDs round-robin by linear id, and each XCD has its own 4 MB
    // L2: with the plain mapping the two N-tiles of one pixel tile (same input!) and the halo-sharing neighbours of a
    // 3x3 conv land on different L2s (measured: 11x the input bytes cross the fabric for the 256->256 head conv).  Give
    // every XCD one contiguous chunk of the tile sequence, N-tile index fastest.
    int mt = bid_x, nt = bid_y;
    {
        const int G = grid_x * grid_y, L = bid_x + grid_x * bid_y;
        if ((G & 7) == 0 && p.xcd_remap) {
            const int tile = (L & 7) * (G >> 3) + (L >> 3);
            mt = tile / grid_y;
            nt = tile - mt * grid_y;
        }
    }
    const int m0 = mt * BM, n0 = nt * BN;
    const bool linear = (p.T == 1 && p.Ho == 0);
    const int kw_n = (p.T == 9) ? 3 : 1;
    const int kc = tid % CH;                         // this thread's chunk column (same for all its rows: 256 % CH == 0)
    const int row0 = tid / CH;                       // first staged row; further rows are +256/CH apart
    constexpr int RSTEP = 256 / CH;
    // LDS-DMA staging (tiles with BN >= 128: the MFMA-bound layers): `buffer_load_dwordx4 ... lds` writes 64 lanes x 16 bytes
    // to LDS at a wave-uniform base + lane * 16, with no VGPR destination and no ds_write.  The lanes of a wave stage 64/CH
    // consecutive rows x CH chunks, which is exactly lane-linear in the unpadded [row][BK] tile; the XOR swizzle therefore moves
    // to the SOURCE side: the lane at physical chunk position kc fetches logical chunk kc ^ swz(row) (the fragment reads are
    // unchanged; swz depends on row bits below the row step, so one value per thread).  Frees 24-44 VGPRs per tile variant.
    constexpr bool DMA = (BN >= 128);
    const int kcg = DMA ? (kc ^ swz<BK>(row0)) : kc;   // chunk index on the global side (swz depends on row bit 3 only: same for row0 + 64 i)

    const auto rx = MAKE_RSRC(p.x);
    const auto rw = MAKE_RSRC(p.w);

    // Stride-2 data gradient (dilated gather): only the taps whose parity matches the output pixel's contribute -- 1, 2, 2 or 4 of the 9,
    // by parity class (oy & 1, ox & 1).  With p.dil_group the GEMM rows enumerate the output pixels class by class (class-major, then
    // sample, then row, then column of the class), so that a tile of BM rows lies in ONE class (except where two classes meet) and the
    // K loop runs over that class's taps only: 2.25 K-steps per channel chunk on average instead of 9 (the other 6.75 multiplied zeros).
    const bool grouped = !linear && p.dilated && p.dil_group;
    const int gny0 = (p.Ho + 1) >> 1, gny1 = p.Ho >> 1, gnx0 = (p.Wo + 1) >> 1, gnx1 = p.Wo >> 1, gB = grouped ? p.M / (p.Ho * p.Wo) : 0;
    const int gs1 = gB * gny0 * gnx0, gs2 = gs1 + gB * gny0 * gnx1, gs3 = gs2 + gB * gny1 * gnx0;      // first row of classes (0,1), (1,0), (1,1)
    auto group_class = [&](int m) { return (m >= gs1 ? 1 : 0) + (m >= gs2 ? 1 : 0) + (m >= gs3 ? 1 : 0); };
    const bool small_m24 = p.M < (1 << 24);          // exact range of fast_div24
    auto idiv = [&](int q, int d) { return small_m24 ? fast_div24(q, d, 1.f / (float)d) : q / d; };
    auto group_pixel = [&](int m, int& b, int& oy, int& ox) {
        const int c = group_class(m), cy = c >> 1, cx = c & 1;
        const int ny = cy ? gny1 : gny0, nx = cx ? gnx1 : gnx0;
        const int r = m - (c == 0 ? 0 : (c == 1 ? gs1 : (c == 2 ? gs2 : gs3)));
        b = idiv(r, ny * nx);
        const int r2 = r - b * ny * nx, y = idiv(r2, nx);
        oy = 2 * y + cy;
        ox = 2 * (r2 - y * nx) + cx;
    };
    unsigned tapmask = 0x1ffu;          // taps this tile walks (bit kh * 3 + kw)
    if (grouped) {
        const int c0 = group_class(m0), c1 = group_class(min(m0 + BM, p.M) - 1);
        if (c0 == c1) {                 // input index = (oy + kh - 1) / 2 must be whole: kh = 1 for even oy, kh in {0, 2} for odd oy
            const unsigned rows = (c0 >> 1) ? 0x5u : 0x2u, cols = (c0 & 1) ? 0x5u : 0x2u;
            tapmask = 0;
            for (int kh = 0; kh < 3; ++kh)
                if (rows >> kh & 1) tapmask |= cols << (3 * kh);
        }
    }
    // ---- fixed per-thread row descriptors
    int a_base[A_PT], a_iy[A_PT], a_ix[A_PT];
    bool a_ok[A_PT];
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
        const int m = m0 + row0 + RSTEP * i;
        a_ok[i] = m < p.M;
        a_base[i] = 0; a_iy[i] = 0; a_ix[i] = 0;
        if (a_ok[i]) {
            if (linear) {
                const int src = p.a_rowmap ? p.a_rowmap[m] : m;
                a_ok[i] = src >= 0;
                a_base[i] = src * p.Cin;
            } else {
                int b, oy, ox;
                if (grouped) {
                    group_pixel(m, b, oy, ox);
                } else {
                    const int hw = p.Ho * p.Wo;
                    b = idiv(m, hw);
                    const int r = m - b * hw;
                    oy = idiv(r, p.Wo);
                    ox = r - oy * p.Wo;
                }
                a_iy[i] = oy * p.stride - p.pad;
                a_ix[i] = ox * p.stride - p.pad;
                a_base[i] = b * p.Hs * p.Ws * p.Cin;
            }
        }
    }
    // Plain convolutions (LEAN = 3): per staged row ONE signed byte offset of its (virtual) top-left tap and a 9-bit mask of the taps that
    // fall inside the image; a tap change is then a scalar delta + bit test + select per row instead of re-deriving and bounds-checking
    // (iy, ix) with divergent branches (~35 instructions per row, on every K-step for 64-channel inputs).
    int a_off0[A_PT];
    unsigned a_tmask[A_PT];
    if (LEAN == 3 && !linear) {
#pragma unroll
        for (int i = 0; i < A_PT; ++i) {
            a_off0[i] = (a_base[i] + (a_iy[i] * p.Ws + a_ix[i]) * p.Cin + kcg * 8) * 2;
            unsigned mk = 0u;
            if (a_ok[i]) {
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw)
                        if (kh < kw_n && kw < kw_n && a_iy[i] + kh >= 0 && a_iy[i] + kh < p.Hs && a_ix[i] + kw >= 0 && a_ix[i] + kw < p.Ws)
                            mk |= 1u << (kh * kw_n + kw);
            }
            a_tmask[i] = mk;
        }
    }
    unsigned b_off[B_PT];
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
        const int q = tid + 256 * i, n = n0 + q / CH;
        b_off[i] = (q < BN * CH && n < p.N) ? (unsigned)((n * p.T * p.Cin + kcg * 8) * 2) : OOB_OFF;
    }
    const int kchunks = (p.Cin + BK - 1) / BK;
    const int nk = (grouped ? __builtin_popcount(tapmask) : p.T) * kchunks;
    auto next_tap = [&](int t) {          // the next tap after t that this tile walks
        ++t;
        if (grouped) {                    // first set bit of the tap mask at or above t (a `while` here was unrolled x8 into ~120 scalar
            const unsigned m = tapmask >> t;                                  // instructions in the K loop of every stride-2 data gradient)
            t = m ? t + __builtin_ctz(m) : 9;
        }
        return t;
    };
    const int t_first = grouped ? next_tap(-1) : 0;

    unsigned a_voff[A_PT];           // byte offset of (row, current tap, channel kc*8), or OOB
    auto set_tap = [&](int t) {
        if (LEAN == 3 && !linear) {
            const int kh3 = kw_n == 3 ? (t * 11) >> 5 : 0, kw3 = t - kh3 * kw_n;          // t / 3 for t < 9
            const int delta = (kh3 * p.Ws + kw3) * p.Cin * 2;
#pragma unroll
            for (int i = 0; i < A_PT; ++i) a_voff[i] = ((a_tmask[i] >> t) & 1u) ? (unsigned)(a_off0[i] + delta) : OOB_OFF;
            return;
        }
        const int kh = kw_n == 3 ? (t * 11) >> 5 : 0, kw = t - kh * kw_n;          // t / 3 for t < 9 (no integer division in the loop)
        if (linear) {
#pragma unroll
            for (int i = 0; i < A_PT; ++i) a_voff[i] = a_ok[i] ? (unsigned)((a_base[i] + kcg * 8) * 2) : OOB_OFF;
            return;
        }
        // branch-free per row (the nested ifs compiled to a divergent branch pair per row and condition: ~35 instructions per row)
        const int dsh = p.dilated ? 1 : 0;
#pragma unroll
        for (int i = 0; i < A_PT; ++i) {
            const int sy = a_iy[i] + kh, sx = a_ix[i] + kw;
            const int iy = sy >> dsh, ix = sx >> dsh;
            const bool ok = a_ok[i] & ((((sy | sx) & dsh) == 0)) & ((unsigned)iy < (unsigned)p.Hs) & ((unsigned)ix < (unsigned)p.Ws);
            a_voff[i] = ok ? (unsigned)((a_base[i] + (iy * p.Ws + ix) * p.Cin + kcg * 8) * 2) : OOB_OFF;
        }
    };
    constexpr bool DEEP = (BN >= 128 && BK == 64 && !DMA);    // global loads issued TWO tiles ahead (second register set), see the main loop
    // Fragment double-buffering (below) and the second global-load register set together need > 256 registers (occupancy 1:
    // head conv 526 us).  Measured one at a time on the 3x3 256->256 head conv (fwd / dgrad): neither 370 / 308 us, fragment
    // prefetch 352 / 302 us, deep global prefetch 359 / 302 us -- both hide latency, neither removes the ceiling of this
    // tiling (64x64 wave tiles: 768 LDS cycles per 512 MFMA cycles and K-step).  The deep variant is kept for BK = 64.
    constexpr bool FRAG_PREFETCH = !DEEP;
    u32x4 ra[A_PT], rb[B_PT], ra2[DEEP ? A_PT : 1], rb2[DEEP ? B_PT : 1];
    auto dma_tiles = [&](int buf, int t, int c0) {       // global -> LDS without registers (DMA variant only)
#if defined(__HIP_DEVICE_COMPILE__)    // the builtin needs a gfx950 target feature: the host pass of hipcc must not see it
        c0 = __builtin_amdgcn_readfirstlane(c0);
        t = __builtin_amdgcn_readfirstlane(t);
        const bool c_ok = (c0 + kcg * 8) < p.Cin;
#pragma unroll
        for (int i = 0; i < A_PT; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(&sA[buf * BM * BK + (wave * (64 / CH) + RSTEP * i) * BK]),
                                                     16, c_ok ? a_voff[i] : OOB_OFF, c0 * 2, 0, 0);
#pragma unroll
        for (int i = 0; i < B_PT; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(&sB[buf * BN * BK + (wave * (64 / CH) + RSTEP * i) * BK]),
                                                     16, c_ok ? b_off[i] : OOB_OFF, (t * p.Cin + c0) * 2, 0, 0);
#endif
    };
    auto load_tiles = [&](u32x4* ra, u32x4* rb, int t, int c0) {       // c0: first channel of this K-chunk (wave-uniform)
        c0 = __builtin_amdgcn_readfirstlane(c0);        // scalar offset operands of the loads below: SGPRs, not a waterfall loop per load
        t = __builtin_amdgcn_readfirstlane(t);
        const bool c_ok = (c0 + kcg * 8) < p.Cin;
#pragma unroll
        for (int i = 0; i < A_PT; ++i)
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, c_ok ? a_voff[i] : OOB_OFF, c0 * 2, 0);
#pragma unroll
        for (int i = 0; i < B_PT; ++i)
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rw, c_ok ? b_off[i] : OOB_OFF, (t * p.Cin + c0) * 2, 0);
    };
    auto store_tiles = [&](const u32x4* ra, const u32x4* rb, int buf) {
#pragma unroll
        for (int i = 0; i < A_PT; ++i) {
            const int row = row0 + RSTEP * i;
            *reinterpret_cast<u32x4*>(&sA[buf * BM * BK + row * BK + ((kc ^ swz<BK>(row)) * 8)]) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < B_PT; ++i) {
            const int q = tid + 256 * i, row = q / CH;
            if (q < BN * CH) *reinterpret_cast<u32x4*>(&sB[buf * BN * BK + row * BK + ((kc ^ swz<BK>(row)) * 8)]) = rb[i];
        }
    };

    f32x4 acc[NI][MI];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < MI; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int t_next = __builtin_amdgcn_readfirstlane(t_first), c_next = 0;     // (tap, chunk) of the tile being loaded
    // (Measured and dropped: chunk-major order -- all nine taps of one channel chunk back to back, so that the shifted re-reads of the
    // same pixels stay in L2 instead of cycling ~11 MB per XCD between two taps (PMC: the head conv fetches 4.1x its input).  The row
    // offsets must then be recomputed every step: head conv forward 335 -> 400 us, dgrad 290 -> 360 us; only N = 32 tiles gained.)
    // ... kept for BN = 32 with nine taps and >= 128 input channels (p.chunk_major, set by igemm_launch): 3x3 256 -> 32 @64x48 fetched
    // 681 MB for its 100 MB input at 5.8 TB/s of fabric traffic, 118 us.)
    // (tap, chunk) are the same for every lane, but the compiler's divergence analysis loses that across the lambdas: it kept c_next in a
    // VGPR, compared it with VALU instructions and -- since it is the scalar offset operand of every staging load -- wrapped EACH buffer load
    // of the K loop in a waterfall loop (v_readfirstlane / v_cmp_eq / s_and_saveexec / load / branch).  An explicit readfirstlane after every
    // update makes them SGPR values again: scalar compares, scalar branches, plain loads.
    auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    auto advance = [&]() {                // next (tap, chunk) in contraction order; recomputes the row offsets on a tap change
        if (BN == 32 && p.chunk_major) {
            if (++t_next == p.T) {
                t_next = 0;
                c_next += BK;
            }
            t_next = uni(t_next);
            c_next = uni(c_next);
            set_tap(t_next);
            return;
        }
        c_next = uni(c_next + BK);
        if (c_next >= p.Cin) {
            c_next = 0;
            t_next = uni(next_tap(t_next));
            set_tap(t_next);
        }
    };
    const int frow = lane & 15, fkc = lane >> 4;
    auto compute = [&](int buf) {
        // (Measured and dropped for the DMA tiles: fragment reads through inline assembly, as in the weight-gradient rings below, so
        // that the compiler's `s_waitcnt vmcnt(0)` in front of the first ds_read -- it cannot prove that the tile requested a moment
        // ago is a different LDS buffer -- disappears and a workgroup overlaps its own loads with its own MFMAs: head conv forward
        // 293 -> 327 us, dgrad 264 -> 273 us.  With two workgroups per CU the other workgroup already covers the loads, and the
        // hand-placed lgkmcnt(0) fences schedule worse than the compiler's counted waits.  The bound of this tiling is LDS read
        // bandwidth: 12 fragment reads per 32 MFMAs and wave (16x16x32 tiles); a 32x32x16 tiling would halve it.)
        if constexpr (BN >= 128 && KS == 2 && FRAG_PREFETCH) {
            // All fragments of the staged tile are read up front into separate registers (KS x (NI + MI) x 4 VGPRs; the kernel
            // sits at 2 waves/SIMD either way) and the scheduler is told to interleave the second K-step's LDS reads with the
            // first K-step's MFMAs: left alone it recycled six fragment registers and exposed an LDS round trip every 4-8 MFMAs.
            bf16x8 wf[KS][NI], af[KS][MI];
    #pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
    #pragma unroll
                for (int a = 0; a < NI; ++a) {
                    const int row = wn * (BN / WN) + a * 16 + frow;
                    wf[ks][a] = *reinterpret_cast<const bf16x8*>(&sB[buf * BN * BK + row * BK + (((fkc + 4 * ks) ^ swz<BK>(row)) * 8)]);
                }
    #pragma unroll
                for (int b = 0; b < MI; ++b) {
                    const int row = wm * (BM / WM) + b * 16 + frow;
                    af[ks][b] = *reinterpret_cast<const bf16x8*>(&sA[buf * BM * BK + row * BK + (((fkc + 4 * ks) ^ swz<BK>(row)) * 8)]);
                }
            }
    #pragma unroll
            for (int ks = 0; ks < KS; ++ks)
    #pragma unroll
                for (int a = 0; a < NI; ++a)
    #pragma unroll
                    for (int b = 0; b < MI; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][a], af[ks][b], acc[a][b], 0, 0, 0);
            if (KS == 2 && NI * MI >= 8) {
                __builtin_amdgcn_sched_group_barrier(0x100, NI + MI, 0);                 // DS reads: fragments of K-step 0
    #pragma unroll
                for (int g = 0; g < (NI + MI) / 2; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, (NI * MI) / ((NI + MI) / 2), 0);   // a few MFMAs of K-step 0 ...
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                              // ... then two reads of K-step 1
                }
                __builtin_amdgcn_sched_group_barrier(0x008, NI * MI, 0);                 // MFMAs of K-step 1
            }
        } else {       // smaller tiles: the extra fragment registers cost a wave of occupancy (measured: slower)
    #pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 wf[NI], af[MI];
    #pragma unroll
                for (int a = 0; a < NI; ++a) {
                    const int row = wn * (BN / WN) + a * 16 + frow;
                    wf[a] = *reinterpret_cast<const bf16x8*>(&sB[buf * BN * BK + row * BK + (((fkc + 4 * ks) ^ swz<BK>(row)) * 8)]);
                }
    #pragma unroll
                for (int b = 0; b < MI; ++b) {
                    const int row = wm * (BM / WM) + b * 16 + frow;
                    af[b] = *reinterpret_cast<const bf16x8*>(&sA[buf * BM * BK + row * BK + (((fkc + 4 * ks) ^ swz<BK>(row)) * 8)]);
                }
    #pragma unroll
                for (int a = 0; a < NI; ++a)
    #pragma unroll
                    for (int b = 0; b < MI; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a], af[b], acc[a][b], 0, 0, 0);
            }
        }
    };
    set_tap(t_first);
    if constexpr (DMA) {
        static_assert(BM % RSTEP == 0 && BN % RSTEP == 0 && (RSTEP % 16) == 0, "lane-linear LDS-DMA layout: whole 1-KiB pieces per wave instruction");
        // (Tried on top: three LDS stages, loads two tiles ahead, one raw s_barrier per K-step with a counted `s_waitcnt vmcnt(6)`
        // so the DMA stays in flight across the barrier -- correct, but 313 / 270 us instead of 304 / 264 us: at two workgroups
        // per CU the other workgroup already covers the load latency; the remaining bound is LDS bandwidth.  The same pipeline on
        // a 256 x 256 tile with 128 x 128 per wave (a third less LDS traffic again, one wave per SIMD): correct, but 256 + 256
        // registers are not enough -- 796 bytes of scratch per lane, 417 / 316 us.)
        dma_tiles(0, t_first, 0);
        __syncthreads();                              // drains vmcnt(0): tile 0 is in LDS
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) {
                advance();
                dma_tiles(buf ^ 1, t_next, c_next);   // the other buffer was last read before the barrier that ended step kt-1
            }
            compute(buf);
            __syncthreads();
        }
    } else {
    load_tiles(ra, rb, t_first, 0);
    store_tiles(ra, rb, 0);
    if constexpr (!DEEP) {
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            const bool more = kt + 1 < nk;
            if (more) {
                advance();
                load_tiles(ra, rb, t_next, c_next);
            }
            compute(buf);
            if (more) store_tiles(ra, rb, buf ^ 1);
            __syncthreads();
        }
    } else {
        // Prefetch distance 2: while tile kt is multiplied out of LDS, tile kt+1 is already in flight into one register set
        // and tile kt+2 is requested into the other; a set is written to LDS a full iteration after its loads were issued
        // (one iteration = 32 MFMAs ~ 0.25 us covers an L2 hit but not an HBM / Infinity-Cache access, and the SQ counters
        // showed 30 % of the wave cycles parked on s_waitcnt).  Unrolled by two so both sets are indexed statically.
        if (nk > 1) {
            advance();
            load_tiles(ra2, rb2, t_next, c_next);           // tile 1 -> set 2
        }
        __syncthreads();
        for (int kt = 0; kt < nk; kt += 2) {
            if (kt + 2 < nk) {
                advance();
                load_tiles(ra, rb, t_next, c_next);          // tile kt+2 -> set 1
            }
            compute(0);
            if (kt + 1 < nk) store_tiles(ra2, rb2, 1);       // tile kt+1 (requested one iteration ago) -> LDS buffer 1
            __syncthreads();
            if (kt + 1 >= nk) break;
            if (kt + 3 < nk) {
                advance();
                load_tiles(ra2, rb2, t_next, c_next);        // tile kt+3 -> set 2
            }
            compute(1);
            if (kt + 2 < nk) store_tiles(ra, rb, 0);         // tile kt+2 -> LDS buffer 0
            __syncthreads();
        }
    }

    }   // !DMA

    // ---- BatchNorm statistics of the raw fp32 accumulators (rows >= M contribute exact zeros)
    if (p.stats) {
#pragma unroll
        for (int a = 0; a < NI; ++a) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = 0.f, q = 0.f;
#pragma unroll
                for (int b = 0; b < MI; ++b) {
                    const float v = acc[a][b][r];
                    s += v;
                    q += v * v;
                }
                s = row16_sum(s);
                q = row16_sum(q);
                if ((lane & 15) == 0) {
                    const int nl = wn * (BN / WN) + a * 16 + (lane >> 4) * 4 + r;
                    sStat[(wm * BN + nl) * 2] = s;
                    sStat[(wm * BN + nl) * 2 + 1] = q;
                }
            }
        }
        __syncthreads();
        constexpr int GROUPS = BM / STAT_ROWS, WPG = WM / GROUPS;        // statistics tiles per workgroup, wave rows per tile
        static_assert(BM % STAT_ROWS == 0 && WM % GROUPS == 0, "statistics tiles must be whole wave rows");
        for (int e = tid; e < BN * GROUPS; e += 256) {       // (BN * GROUPS may exceed the 256 threads of the workgroup)
            const int g = e / BN, nl = e % BN;
            // a group whose 128 rows all lie at or beyond M has no statistics row (M % 256 in (0, 128] on the 256-row tile: the buffer ends
            // at ceil(M / 128) rows) -- the guard of k_conv8p
            if (n0 + nl >= p.N || m0 + g * STAT_ROWS >= p.M) continue;
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int w = 0; w < WPG; ++w) {
                s += sStat[((g * WPG + w) * BN + nl) * 2];
                q += sStat[((g * WPG + w) * BN + nl) * 2 + 1];
            }
            float* dst = p.stats + (size_t)(mt * GROUPS + g) * 2 * p.N;
            dst[n0 + nl] = s;
            dst[p.N + n0 + nl] = q;
        }
    }

    // ---- epilogue: accumulators -> wave-private fp32 LDS tile -> rolled loop over 8-column row segments
    // (BPP 16-row blocks per pass: all of them for BM = 128; two at a time for the 256-row tile, whose 128 x 64 wave tiles
    // would need 139 KB of staging)
    if (p.stats) __syncthreads();                    // sStat (aliases the staging tile) has been consumed
    float* stage = reinterpret_cast<float*>(smem) + wave * (BPP * 16) * EP;
    constexpr int LPR = TN / 8, RPP = 64 / LPR;      // lanes per row, rows per pass
    const int hw_out = p.Ho * p.Wo;
    const int lr = lane / LPR, lc = (lane % LPR) * 8;
    const int n = n0 + wn * TN + lc;
    const bool n_ok = n < p.N;
    f32x4 blo = {0.f, 0.f, 0.f, 0.f}, bhi = {0.f, 0.f, 0.f, 0.f};     // the lane's columns are the same in every pass
    if (p.bias && n_ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n + j < p.N) blo[j] = p.bias[n + j];
            if (n + 4 + j < p.N) bhi[j] = p.bias[n + 4 + j];
        }
    }
    f32x4 slo = {1.f, 1.f, 1.f, 1.f}, shi = {1.f, 1.f, 1.f, 1.f};
    if (p.col_scale && n_ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n + j < p.N) slo[j] = p.col_scale[n + j];
            if (n + 4 + j < p.N) shi[j] = p.col_scale[n + 4 + j];
        }
    }
    // The staging tile is wave-private: only the lanes of ONE wave exchange data through it, so a wave-level fence orders the writes
    // against the reads (a workgroup barrier made every wave wait for the slowest of four, twice per pass -- these epilogues are
    // most of the run time of the shallow GEMMs).
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
#pragma unroll
    for (int pass = 0; pass < MI / BPP; ++pass) {
        if (pass) wave_sync();                       // the previous pass has been read out
#pragma unroll
        for (int bb = 0; bb < BPP; ++bb)
#pragma unroll
            for (int a = 0; a < NI; ++a)
                *reinterpret_cast<f32x4*>(&stage[(bb * 16 + (lane & 15)) * EP + a * 16 + (lane >> 4) * 4]) = acc[a][pass * BPP + bb];
        wave_sync();
        if (n_ok) {
#pragma unroll 2
            for (int ps = 0; ps < BPP * 16 / RPP; ++ps) {
                const int ml = ps * RPP + lr;
                const int m = m0 + wm * TM + pass * BPP * 16 + ml;
                int orow = (m < p.M) ? m : -1;
                if (orow >= 0 && p.o_rowmap) orow = p.o_rowmap[m];
                if (orow >= 0 && grouped) {                  // GEMM row of the parity-grouped enumeration -> output pixel row
                    int gb, goy, gox;
                    group_pixel(m, gb, goy, gox);
                    orow = (gb * p.Ho + goy) * p.Wo + gox;
                }
                if (orow < 0) continue;
                const float rs = p.res_scale ? p.res_scale[idiv(orow, p.rows_per_sample)] : 1.f;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(&stage[ml * EP + lc]);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(&stage[ml * EP + lc + 4]);
                igemm_epilogue_row8(p, lo, hi, slo, shi, blo, bhi, orow, n, rs, hw_out);
            }
        }
    }
}

template <int BM, int BN, int WM, int WN, int BK, int LEAN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_igemm2(IgemmArgs p_in) {
    igemm2_body<BM, BN, WM, WN, BK, LEAN>(p_in, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, (int)gridDim.y);
}

// GROUPED launch (round 4): up to PK_GROUP_MAX independent convolutions / linear layers of ONE tile shape in one launch.  The exchange
// units of HRNet / HRFormer (hrformer.py:420-491, hrnet.py:157-227) are 2-12 tiny conv + BatchNorm layers per level on 1 500 .. 50 000
// pixels; as separate launches each paid ~10 us of fixed cost (dispatch ramp, cold code, first-tile latency, epilogue tail) for 1-3 us of
// work, and the step time followed the NUMBER of launches (1 288 x 13 us = 17 ms).  The argument blocks travel BY VALUE in the kernel
// arguments (no descriptor upload: the pointers change every step in eager mode); `first` is the prefix sum of the members' tile counts.
struct IgemmGroup {
    IgemmArgs a[PK_GROUP_MAX];
    int first[PK_GROUP_MAX + 1];
    int gy[PK_GROUP_MAX];
    int n;
};
template <int BM, int BN, int WM, int WN, int BK, int LEAN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_igemm2g(IgemmGroup g) {
    const int L = (int)blockIdx.x;
    PK_GROUP_MEMBER(i, g.first, g.n, L);
    const int local = L - g.first[i], gy = g.gy[i], gx = (g.first[i + 1] - g.first[i]) / gy;
    igemm2_body<BM, BN, WM, WN, BK, LEAN>(g.a[i], local % gx, local / gx, gx, gy);
}

// ================================================================================================ ring kernel (head convs)
// The 3x3 256 -> 256 convolutions of the fusion head (forward and data gradient: 8 launches of 232 GFLOP per step, 65 % of the
// model's flops) on the two-barrier-per-K-step tile above sit at that structure's ceiling (~850 TFLOP/s isolated: every K-step drains
// the LDS-DMA with vmcnt(0) in front of the barrier).  k_conv8p is the deep-pipeline structure instead:
//   * 256 pixels x 256 output channels per 512-thread workgroup (8 waves as 2 (pixels) x 4 (channels), 128 x 64 per wave = 128
//     accumulator registers), one workgroup per CU;
//   * K-tile = 32 channels of one filter tap = one MFMA k-step: [256 pixel rows | 256 weight rows] x 64 bytes = 32 KB, in a FIVE-stage
//     LDS ring (160 KB).  Operands travel global -> LDS by LDS-DMA (4 x 1 KiB pieces per wave and tile, XOR swizzle on the source side)
//     and stay in flight across barriers: tile t+3 is requested while tile t is multiplied, the only vmcnt wait is a counted one
//     (tile t+1 landed, tiles t+2 and t+3 still in flight: two whole steps of latency cover);
//   * per K-tile a wave reads 4 weight + 8 pixel fragments (12 ds_read_b128) and issues 32 MFMAs (16x16x32);
//   * ONE barrier per K-tile.  The two wave groups (waves 0-3 / 4-7: the two waves of every SIMD) run the step in opposite order: between
//     two barriers group 0 does [reads + DMA issue of tile t; 32 MFMAs of tile t], group 1 [32 MFMAs of tile t-1 from the fragments it
//     read in the previous interval; reads + DMA issue of tile t] -- while one wave of a SIMD loads, its partner holds the matrix pipe.
//   (Measured on the way: 64-channel K-tiles in two 64 KB buffers, four quadrant phases of 16 MFMAs and two barriers each, the groups half
//   a phase apart -- 233 us for the head conv's data gradient against 264 us on k_igemm2; ablations on that version: MFMAs + barriers
//   alone 157 us (~100 cycles of barrier overhead per 256-cycle MFMA slot), DMA + reads + barriers alone 174 us.  The ring with two
//   barriers per 32-MFMA step: 211 us.)
//   (Measured and dropped: PERSISTENT workgroups (one per CU walking its share of the output tiles, the K-tile ring continuing across
//   tiles, each wave storing its finished tile straight from the accumulators as 16-byte pieces after a v_permlane16_swap while its
//   partner multiplies) -- 224 / 244 us (data gradient / forward + statistics) against 212 / 229 us for one tile per workgroup with
//   the LDS-staged 128-byte row stores below; launched with one workgroup per tile the same code ran 224 / 255 us, i.e. the three
//   lock-step rounds of 256 workgroups cost nothing, the half-line stores do.  Ablations of this version (data gradient, 210 us):
//   MFMAs + barriers alone 158 us (= the guide's 256 x 256 GEMM rate, i.e. the sustained-clock MFMA ceiling), reads + DMA + barriers
//   alone 145 us, nothing but prologue / barriers / epilogue 56 us.)
// Hazards (J_t = interval between barriers t-1 and t; both groups read tile t and request tile t+3 in J_t):
//   RAW  every wave waits for ITS pieces of tile t+1 (counted vmcnt) before barrier t; the first read of tile t+1 is in J_t+1;
//   WAR  group 1 fences its reads of tile t-2 (lgkmcnt(0)) at the start of J_t-1, group 0 inside J_t-2; the DMA of tile t+3 into the
//        same ring stage is issued in J_t.
// LDS reads of DMA-filled tiles go through inline assembly (see ring_tr above: the compiler would drain the DMA in front of every
// ds_read it can see).  Supported: stride-1 3x3 / 1x1 convolutions, Cin % 32 == 0 with >= 18 K-tiles, N % 256 == 0, bf16 row-major
// output, optional BatchNorm statistics; everything else stays on k_igemm2.
#define C8_STAGE 32768          // bytes per ring stage: [pixels 256 x 64 B | weights 256 x 64 B]
#define C8_STAGES 5
template <int OFF>
__device__ __forceinline__ bf16x8 c8_read(uint32_t lds_byte_addr) {          // OFF: immediate (16-bit) byte offset -- no address VALU per read
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(lds_byte_addr), "n"(OFF) : "memory");
    return v;
}
__device__ __forceinline__ void c8_fence4(bf16x8& a, bf16x8& b, bf16x8& c, bf16x8& d) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
__device__ __forceinline__ void c8_barrier() { asm volatile("s_barrier" ::: "memory"); }

__global__ void __launch_bounds__(512, 2) k_conv8p(IgemmArgs p) {
    __shared__ __attribute__((aligned(1024))) uint16_t c8_smem[C8_STAGES * C8_STAGE / 2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the LDS-DMA destinations (M0) and the group tests are SGPR arithmetic
    const int grp = wave >> 2;                 // wave group = pixel half of the tile (and the half-step stagger)
    const int wn = wave & 3;                   // 64-channel quarter
    // XCD-contiguous tile order (bijective for any grid size): blocks b and b + 8 share an XCD's L2, neighbouring pixel tiles share halo rows
    int mt, nt;
    {
        const int G = gridDim.x, L = blockIdx.x, q = G >> 3, r = G & 7, xcd = L & 7;
        const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
        const int ntiles = p.N >> 8;
        mt = tile / ntiles;
        nt = tile - mt * ntiles;
    }
    const int m0 = mt * 256, n0 = nt * 256;
    const auto rx = MAKE_RSRC(p.x);
    const auto rw = MAKE_RSRC(p.w);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)c8_smem;

    // ---- DMA geometry: a 1 KiB piece = 16 rows x 64 bytes; in the pixel tile and in the weight tile this wave moves pieces wave and
    // 8 + wave, i.e. this thread rows (i * 8 + wave) * 16 + lane / 4, i = 0, 1, physical chunk lane % 4
    const int drow = wave * 16 + (lane >> 2);
    const int lchunk = (lane & 3) ^ (((lane >> 5) & 1) << 1);    // logical chunk fetched into physical position lane % 4: ^ swz<32>(row)
    unsigned pc[2];                                              // byte offset of (pixel, channel lchunk * 8) at the centre tap, or OOB
    int pedge[2];                                                // bit 0: row above exists, 1: below, 2: left, 3: right
    unsigned wo[2];                                              // byte offset of weight row n, tap 0, channel lchunk * 8
    {
        const int hw = p.Ho * p.Wo;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + i * 128 + drow;
            pc[i] = OOB_OFF;
            pedge[i] = 0;
            if (m < p.M) {
                const int b = m / hw, rr = m - b * hw, oy = rr / p.Wo, ox = rr - oy * p.Wo;
                pc[i] = (unsigned)(((b * p.Hs + oy) * p.Ws + ox) * p.Cin + lchunk * 8) * 2u;
                pedge[i] = (oy > 0 ? 1 : 0) | (oy < p.Hs - 1 ? 2 : 0) | (ox > 0 ? 4 : 0) | (ox < p.Ws - 1 ? 8 : 0);
            }
            wo[i] = (unsigned)(((n0 + i * 128 + drow) * p.T) * p.Cin + lchunk * 8) * 2u;
        }
    }
    const int nk = p.T * (p.Cin >> 5);
    // (tap, first channel) of the tile being requested, with the tap's edge requirements and pixel offset (all wave-uniform)
    int q_tap = 0, q_c0 = 0, q_need = 0, q_delta = 0;
    auto set_tap = [&]() {
        if (p.T == 9) {
            const int kh = q_tap / 3, kw = q_tap - kh * 3;
            q_need = (kh == 0 ? 1 : 0) | (kh == 2 ? 2 : 0) | (kw == 0 ? 4 : 0) | (kw == 2 ? 8 : 0);
            q_delta = ((kh - 1) * p.Ws + (kw - 1)) * p.Cin * 2;
        }
    };
    set_tap();
    auto issue_tile = [&](int stage) {          // K-tile (q_tap, q_c0) -> ring stage; then advance to the next K-tile
#if defined(__HIP_DEVICE_COMPILE__)
        uint16_t* sp = c8_smem + (stage * C8_STAGE + wave * 1024) / 2;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool ok = pc[i] != OOB_OFF && (pedge[i] & q_need) == q_need;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(sp + i * 4096), 16,
                                                     ok ? pc[i] + (unsigned)q_delta : OOB_OFF, q_c0 * 2, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(sp + 8192 + i * 4096), 16, wo[i],
                                                     (q_tap * p.Cin + q_c0) * 2, 0, 0);
#endif
        // chunk-major K order: the nine taps of one 32-channel chunk back to back -- the shifted re-reads of the same pixel rows (64
        // bytes each) hit the XCD's L2 instead of cycling the whole 256-channel rows through it between two taps (PMC, tap-major:
        // 394 MB fetched for 100 MB of input).  A tap change costs this kernel two scalars, no per-row address work.
        if (++q_tap == p.T) {
            q_tap = 0;
            q_c0 += 32;
        }
        set_tap();
    };

    // ---- fragment addresses: row (lane & 15) of a 16-row block, logical chunk lane >> 4, swizzled; blocks are 1024 bytes apart
    const int frow = lane & 15;
    const uint32_t fchunk = (uint32_t)(((lane >> 4) ^ ((frow >> 3) << 1)) * 16);
    const uint32_t faddr_p = lds0 + (grp * 128 + frow) * 64 + fchunk;                        // + stage * 32768 + pixel block * 1024
    const uint32_t faddr_w = lds0 + 16384 + (wn * 64 + frow) * 64 + fchunk;                  // + stage * 32768 + channel block * 1024

    f32x4 acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- prologue: tiles 0, 1, 2 requested; tile 0 landed
    issue_tile(0);
    issue_tile(1);
    issue_tile(2);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    c8_barrier();
    int st_r = 0, st_w = 3;                    // ring stage read by this step / filled with tile t + 3
    bf16x8 wf[4], pf[8];
    auto multiply = [&]() {
        c8_fence4(wf[0], wf[1], wf[2], wf[3]);
        c8_fence4(pf[0], pf[1], pf[2], pf[3]);
        c8_fence4(pf[4], pf[5], pf[6], pf[7]);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a], pf[b], acc[a][b], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };
    for (int t = 0; t <= nk; ++t) {
        if (grp == 1 && t > 0) multiply();                         // group 1: tile t-1, from the fragments it read in the previous interval
        if (t < nk) {
            const uint32_t bp = faddr_p + st_r * C8_STAGE, bw = faddr_w + st_r * C8_STAGE;
            wf[0] = c8_read<0>(bw);
            wf[1] = c8_read<1024>(bw);
            wf[2] = c8_read<2048>(bw);
            wf[3] = c8_read<3072>(bw);
            pf[0] = c8_read<0>(bp);
            pf[1] = c8_read<1024>(bp);
            pf[2] = c8_read<2048>(bp);
            pf[3] = c8_read<3072>(bp);
            pf[4] = c8_read<4096>(bp);
            pf[5] = c8_read<5120>(bp);
            pf[6] = c8_read<6144>(bp);
            pf[7] = c8_read<7168>(bp);
            if (t + 3 < nk) issue_tile(st_w);
            __builtin_amdgcn_sched_barrier(0);
            if (grp == 0) multiply();                              // group 0: tile t
        }
        // counted wait: tile t+1 has landed (tiles t+2, t+3 may still be in flight)
        if (t + 3 < nk) {
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else if (t + 2 < nk) {
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        st_r = st_r == C8_STAGES - 1 ? 0 : st_r + 1;
        st_w = st_w == C8_STAGES - 1 ? 0 : st_w + 1;
        c8_barrier();
    }

    // ---- BatchNorm statistics: a wave's 128 pixels are exactly one statistics tile (STAT_ROWS = 128) of its 64 channels.  A wave group
    // whose 128 pixels all lie beyond M writes no row: the buffer has pk_conv_stats_tiles(M) = ceil(M / 128) rows, and the second half of
    // a last tile with M % 256 in (0, 128] would be row ceil(M / 128), past its end.
    if (p.stats && m0 + grp * 128 < p.M) {
        float* dst = p.stats + (size_t)(mt * 2 + grp) * 2 * p.N + n0 + wn * 64;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float sm = 0.f, sq = 0.f;
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const float v = acc[a][b][r];
                    sm += v;
                    sq += v * v;
                }
                sm = row16_sum(sm);
                sq = row16_sum(sq);
                if ((lane & 15) == 0) {
                    const int nl = a * 16 + (lane >> 4) * 4 + r;
                    dst[nl] = sm;
                    dst[p.N + nl] = sq;
                }
            }
    }
    // ---- epilogue: bf16 tile of the wave (128 pixels x 64 channels = 16 KB) through its own LDS slice, 16-byte chunks XOR-swizzled by
    // (pixel & 7); then 128-byte row segments to global, 16 bytes per lane
    uint16_t* stage = c8_smem + wave * 8192;
    if (p.col_scale) {          // eval-mode BatchNorm folded in: y = relu?(scale * conv + shift); channel = n0 + 64 wn + 16 a + 4 (lane >> 4) + r
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int c = n0 + wn * 64 + a * 16 + (lane >> 4) * 4;
            const f32x4 sc = *reinterpret_cast<const f32x4*>(p.col_scale + c), sh = *reinterpret_cast<const f32x4*>(p.bias + c);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                acc[a][b] = acc[a][b] * sc + sh;
                if (p.act == 3) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[a][b][r] = fmaxf(acc[a][b][r], 0.f);
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int px = b * 16 + (lane & 15);
            const int chunk = (a * 2 + (lane >> 5)) ^ (px & 7);
            uint2 v;
            v.x = pack_bf16x2(acc[a][b][0], acc[a][b][1]);
            v.y = pack_bf16x2(acc[a][b][2], acc[a][b][3]);
            *reinterpret_cast<uint2*>(stage + px * 64 + chunk * 8 + ((lane >> 4) & 1) * 4) = v;
        }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint16_t* out = reinterpret_cast<uint16_t*>(p.out);
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
        const int px = it * 8 + (lane >> 3), ch = lane & 7;
        const int m = m0 + grp * 128 + px;
        const u32x4 v = *reinterpret_cast<const u32x4*>(stage + px * 64 + ((ch ^ (px & 7)) * 8));
        if (m < p.M) *reinterpret_cast<u32x4*>(out + (size_t)m * p.ldo + n0 + wn * 64 + ch * 8) = v;
    }
}
// ================================================================================================ halo kernel (small-channel 3x3 convs)
// 3x3 stride-1 convolutions with 32 / 64 input and output channels on large maps (layer1, transitions and exchange units of HRFormer,
// every BasicBlock of HRNet's high-resolution branches) are HBM-bound by arithmetic (64 -> 64 @64x48: 50 MB, 14.5 GFLOP) but ran at
// 0.14 of the MFMA peak on k_igemm2: every tap re-stages the 128-row input tile through registers and LDS (9x the input through the
// L2 -> LDS path, ~8 TB/s) and every workgroup re-reads the weights.  k_conv3h:
//   * the K loop runs over PADDED pixel positions q = (b, py, px) of the zero-bordered (H+2) x (W+2) image (the trick of k_wgrad4_3x3):
//     out[q] = sum_taps X[q + (kh-1)(W+2) + (kw-1)] . W[tap], so every tap of a tile of 128 consecutive positions is the SAME LDS tile read
//     at a row offset -- the input tile plus a (W+3)-row halo either side goes global -> LDS ONCE per tile, by LDS-DMA, border positions
//     fetched with the out-of-range offset (zeros); border outputs are computed and dropped;
//   * the weights of a wave's output columns (all nine taps) live in REGISTERS for the whole kernel (144 VGPRs at 64 -> 64): waves as
//     2 (positions) x 2 (channels), 64 positions x COUT/2 channels each;
//   * persistent workgroups (two per CU) walk the tiles of one XCD's contiguous range; the DMA of tile i+1 flies under the MFMAs of tile i
//     (two LDS buffers, one counted wait + two barriers per tile);
//   * fragment addresses do not depend on the tile: nine per-tap base addresses per lane, computed once (the XOR swizzle term of a row is
//     the same for all four 16-row blocks of a wave and both k-steps differ by one address bit).
// Epilogue straight from the accumulators: interior positions only, optional addend; the BatchNorm statistics of a wave are kept in
// registers over all its tiles and written once (one partial row per workgroup and position half: pk_conv_stats_rows).
// Measured (B = 64, rocprof): 64 -> 64 @64x48 43.5 -> 30.8 us, @48x36 33 -> 22, 32 -> 32 @96x72 (B = 64) 38.5 -> 24.5, @16x12 15.3 -> 11.4.
// Batch sweep of 64 -> 64 @64x48 (17.1 / 22.4 / 30.8 / 45.2 / 77.3 us at B = 16 / 32 / 64 / 128 / 256): ~11 us fixed (launch, 75 MB of
// weight fragments into 2 048 waves' registers, first tiles' DMA, last stores) + ~5 us per tile slot; at B = 64 a workgroup walks 3 or
// 4 tiles (1 650 tiles on 512 workgroups), so a quarter of the loop time is the fourth-tile tail.  Tried without effect: double-buffered
// fragment reads (the LDS latency is hidden by the other workgroup of the CU), carried instead of divided DMA row coordinates, letting
// a tile's stores drain under the next two tiles (kept: it is free), retiring the weight loads in front of the loop (kept: without it
// the compiler's lazy waits sit inside the MFMA stream).
template <int OFF>
__device__ __forceinline__ bf16x8 h3_read(uint32_t lds_byte_addr) {
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(lds_byte_addr), "n"(OFF) : "memory");
    return v;
}
// s_waitcnt vmcnt(n) with a wave-uniform run-time n (the immediate is 6 bits: n > 63 waits for less than asked, which is always safe)
__device__ __forceinline__ void h3_wait_vm(int n) {
#define H3_W(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n < 0 ? 0 : (n > 63 ? 63 : n)) {
        H3_W(0) H3_W(1) H3_W(2) H3_W(3) H3_W(4) H3_W(5) H3_W(6) H3_W(7) H3_W(8) H3_W(9) H3_W(10) H3_W(11) H3_W(12) H3_W(13) H3_W(14) H3_W(15)
        H3_W(16) H3_W(17) H3_W(18) H3_W(19) H3_W(20) H3_W(21) H3_W(22) H3_W(23) H3_W(24) H3_W(25) H3_W(26) H3_W(27) H3_W(28) H3_W(29) H3_W(30) H3_W(31)
        H3_W(32) H3_W(33) H3_W(34) H3_W(35) H3_W(36) H3_W(37) H3_W(38) H3_W(39) H3_W(40) H3_W(41) H3_W(42) H3_W(43) H3_W(44) H3_W(45) H3_W(46) H3_W(47)
        H3_W(48) H3_W(49) H3_W(50) H3_W(51) H3_W(52) H3_W(53) H3_W(54) H3_W(55) H3_W(56) H3_W(57) H3_W(58) H3_W(59) H3_W(60) H3_W(61) H3_W(62) H3_W(63)
    }
#undef H3_W
}
template <int CIN, int COUT>
__global__ void __launch_bounds__(256, 2) k_conv3h(IgemmArgs p, int pieces_per_wave) {
    constexpr int RB = CIN * 2, CH = CIN / 8, RP = 1024 / RB, KS = CIN / 32, NI = COUT / 32;
    extern __shared__ __attribute__((aligned(1024))) uint16_t h3_smem[];          // [2][pieces_per_wave * 4 KiB]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int H = p.Hs, W = p.Ws, W2 = W + 2, P = (H + 2) * W2, halo = W + 3;
    const int nsamples = p.M / (H * W), Mp = nsamples * P;                        // padded positions of the whole batch
    const int ntiles = (Mp + 127) >> 7;
    const float invP = 1.f / (float)P, invW2 = 1.f / (float)W2;
    const int bufbytes = pieces_per_wave * 4096;
    // persistent workgroups, XCD-contiguous tile ranges (neighbouring tiles share their halo rows in L2)
    int tile_first, tile_step, n_mine;
    {
        const int G = gridDim.x, L = blockIdx.x, q = ntiles >> 3, r = ntiles & 7, x = L & 7, j = L >> 3;
        const int start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q, cnt = q + (x < r ? 1 : 0);
        tile_step = (G - x + 7) >> 3;
        tile_first = start + j;
        n_mine = j < cnt ? (cnt - j + tile_step - 1) / tile_step : 0;
    }
    if (n_mine == 0) {          // (uneven XCD ranges can leave a workgroup without a tile: its statistics rows are zeros)
        if (p.stats)
            for (int i = tid; i < 4 * COUT; i += 256) p.stats[(size_t)blockIdx.x * 4 * COUT + i] = 0.f;
        return;
    }
    const auto rx = MAKE_RSRC(p.x);
    const auto ro = MAKE_RSRC((uint16_t*)p.out);
    const auto rr = MAKE_RSRC(p.res ? p.res : p.x);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)h3_smem;

    // ---- per-tap fragment base addresses (bytes from the start of a buffer): LDS row halo + 64 wm + (lane & 15) + tap offset, chunk lane >> 4
    uint32_t fa[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int kh = t / 3, kw = t - kh * 3;
        const int row = halo + wm * 64 + (lane & 15) + (kh - 1) * W2 + (kw - 1);
        const int sw = CIN == 64 ? ((row >> 1) & 7) : (((row >> 3) & 1) << 1);
        fa[t] = lds0 + (uint32_t)(row * RB + (((lane >> 4) ^ sw) & (CH - 1)) * 16);
    }
    // ---- DMA of the input tile + halo: buffer row j <-> padded position q0 - halo + j; 1 KiB pieces of RP rows, piece = wave + 4 i
    const int prow = lane / CH, pchunk = lane % CH;
    auto issue_tile = [&](int tile, int buf) {
#if defined(__HIP_DEVICE_COMPILE__)
        // (b, py, px) of this lane's row in its first piece by two divisions, then carried from piece to piece (+ 4 RP positions)
        const int q = tile * 128 - halo + wave * RP + prow;
        int b = fast_div24(q, P, invP);
        const int rem = q - b * P;
        int py = fast_div24(rem, W2, invW2), px = rem - py * W2;
        for (int i = 0; i < pieces_per_wave; ++i) {
            const int piece = wave + 4 * i, j = piece * RP + prow;
            const int sw = CIN == 64 ? ((j >> 1) & 7) : (((j >> 3) & 1) << 1);
            const bool ok = b >= 0 && b < nsamples && py >= 1 && py <= H && px >= 1 && px <= W;
            const unsigned off = ok ? (unsigned)((((b * H + py - 1) * W + px - 1) * CIN + ((pchunk ^ sw) & (CH - 1)) * 8) * 2) : OOB_OFF;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(h3_smem + (buf * bufbytes + piece * 1024) / 2), 16, off, 0, 0, 0);
            px += 4 * RP;
            while (px >= W2) {
                px -= W2;
                if (++py == H + 2) {
                    py = 0;
                    ++b;
                }
            }
        }
#endif
    };
    f32x4 acc[NI][4];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float ssum[NI][4], ssq[NI][4];              // BatchNorm statistics of this wave over ALL its tiles (lane: position lane % 16, channels 4 g ..)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) ssum[ni][r] = ssq[ni][r] = 0.f;
    // Vector-memory operations of one wave, in issue order: DMA(0) DMA(1) | DMA(2) ST(0) | DMA(3) ST(1) | ...  (iteration i computes tile
    // i, then requests tile i+2 into the buffer it has just read, then stores tile i).  vmcnt counts loads AND stores in order, so the
    // wait for DMA(i) at the top of iteration i names what may stay in flight behind it -- ST(i-2), DMA(i+1), ST(i-1): a tile's stores
    // drain under the NEXT TWO tiles' MFMAs instead of stalling the next iteration (first version: wait for everything but DMA(i+1) --
    // each tile paid an HBM write round trip).
    // (only the NI * 4 output stores per tile are counted -- buffer-store intrinsics the backend cannot merge; the statistics stores and
    // addend loads on top of them make the wave wait for MORE than it must, never less)
    constexpr int n_st = NI * 4;
    issue_tile(tile_first, 0);
    if (n_mine > 1) issue_tile(tile_first + tile_step, 1);
    // (the weight loads go out BEHIND the first two tiles' DMA: one memory round trip for both instead of two in a row)
    // ---- weights of this wave's COUT/2 output channels, all nine taps, as MFMA A fragments (row = channel, 8 k-values per lane)
    bf16x8 wreg[9][KS][NI];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int n = wn * (COUT / 2) + ni * 16 + (lane & 15);
                wreg[t][ks][ni] = *reinterpret_cast<const bf16x8*>(p.w + ((size_t)n * 9 + t) * CIN + ks * 32 + (lane >> 4) * 8);
            }
    // The weight loads are retired HERE, through an asm that redefines every fragment: otherwise the compiler waits for them lazily at
    // their first use INSIDE the tile loop -- counted vmcnt waits that, from the second tile on, wait for the DMA of the next tile and the
    // stores of the previous one in the middle of the MFMAs (first version: 32 us, the DMA never overlapped the compute).
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) asm volatile("s_waitcnt vmcnt(0)" : "+v"(wreg[t][ks][ni])::"memory");
    for (int it = 0; it < n_mine; ++it) {
        const int tile = tile_first + it * tile_step, buf = it & 1;
        {
            int allow = 0;                                  // operations issued after DMA(it)
            if (it + 1 < n_mine) allow += pieces_per_wave;  // DMA(it+1)
            if (it >= 1) allow += n_st;                     // ST(it-1)
            if (it >= 2) allow += n_st;                     // ST(it-2)
            h3_wait_vm(allow);
        }
        asm volatile("s_barrier" ::: "memory");
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[ni][b] = zero;
        const uint32_t boff = (uint32_t)(buf * bufbytes);
        // 9 * KS steps of [4 fragment reads | 4 NI MFMAs]; the reads of step s+1 are issued before the MFMAs of step s (two fragment sets,
        // a counted lgkmcnt(4) keeps the younger four in flight): the LDS latency of every step was exposed otherwise
        bf16x8 pf[2][4];
        {
            const uint32_t a = fa[0] + boff;
            pf[0][0] = h3_read<0>(a);
            pf[0][1] = h3_read<16 * RB>(a);
            pf[0][2] = h3_read<32 * RB>(a);
            pf[0][3] = h3_read<48 * RB>(a);
        }
#pragma unroll
        for (int st = 0; st < 9 * KS; ++st) {
            const int t = st / KS, ks = st % KS, cur = st & 1;
            if (st + 1 < 9 * KS) {
                const int t2 = (st + 1) / KS, ks2 = (st + 1) % KS;
                const uint32_t a = (fa[t2] + boff) ^ (ks2 ? 64u : 0u);
                pf[cur ^ 1][0] = h3_read<0>(a);
                pf[cur ^ 1][1] = h3_read<16 * RB>(a);
                pf[cur ^ 1][2] = h3_read<32 * RB>(a);
                pf[cur ^ 1][3] = h3_read<48 * RB>(a);
                asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(pf[cur][0]), "+v"(pf[cur][1]), "+v"(pf[cur][2]), "+v"(pf[cur][3])::"memory");
            } else {
                c8_fence4(pf[cur][0], pf[cur][1], pf[cur][2], pf[cur][3]);
            }
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[ni][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[t][ks][ni], pf[cur][b], acc[ni][b], 0, 0, 0);
        }
        asm volatile("s_barrier" ::: "memory");          // every wave has finished reading this buffer ...
        if (it + 2 < n_mine) issue_tile(tile + 2 * tile_step, buf);      // ... tile it+2 is requested into it
        // ---- epilogue: lane (row g = lane / 16, position lane % 16 of block b) holds channels 16 ni + 4 g .. + 3; interior positions only
        const int g = lane >> 4;
        // (b, py, px) of this lane's position in block 0 by two divisions, carried to blocks 1-3 (+ 16 positions each)
        int eb, epy, epx;
        {
            const int q = tile * 128 + wm * 64 + (lane & 15);
            eb = fast_div24(q, P, invP);
            const int rem = q - eb * P;
            epy = fast_div24(rem, W2, invW2);
            epx = rem - epy * W2;
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const bool ok = eb < nsamples && epy >= 1 && epy <= H && epx >= 1 && epx <= W;
            const int m = (eb * H + epy - 1) * W + epx - 1;
            epx += 16;
            while (epx >= W2) {
                epx -= W2;
                if (++epy == H + 2) {
                    epy = 0;
                    ++eb;
                }
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                f32x4 v = acc[ni][b];
                if (p.stats && ok) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        ssum[ni][r] += v[r];
                        ssq[ni][r] += v[r] * v[r];
                    }
                }
                const unsigned off = ok ? (unsigned)(m * COUT + wn * (COUT / 2) + ni * 16 + g * 4) * 2u : OOB_OFF;
                if (p.col_scale) {          // eval-mode BatchNorm folded in (scale, shift of this lane's four channels: L1-resident)
                    const int c = wn * (COUT / 2) + ni * 16 + g * 4;
                    v = v * *reinterpret_cast<const f32x4*>(p.col_scale + c) + *reinterpret_cast<const f32x4*>(p.bias + c);
                }
                if (p.res) {
                    const u32x2 rv = __builtin_amdgcn_raw_buffer_load_b64(rr, off, 0, 0);
                    v[0] += bf16_lo(rv[0]); v[1] += bf16_hi(rv[0]); v[2] += bf16_lo(rv[1]); v[3] += bf16_hi(rv[1]);
                }
                if (p.act == 3) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                }
                const u32x2 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
                __builtin_amdgcn_raw_buffer_store_b64(o, ro, off, 0, 0);
            }
        }
    }
    if (p.stats) {          // ONE partial row per (workgroup, position half): the sums of all its tiles, kept in registers until here
        const int g = lane >> 4;
        float* dst = p.stats + (size_t)(blockIdx.x * 2 + wm) * 2 * COUT + wn * (COUT / 2);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sm = row16_sum(ssum[ni][r]), sq = row16_sum(ssq[ni][r]);
                if ((lane & 15) == 0) {
                    dst[ni * 16 + g * 4 + r] = sm;
                    dst[COUT + ni * 16 + g * 4 + r] = sq;
                }
            }
    }
}
// ================================================================================================ routing
// Which kernel, tile and grid a call gets is decided in igemm_route and nowhere else: igemm_launch only maps the route to the instantiation,
// and pk_conv_stats_rows sizes the statistics buffer from the same route.  Every threshold sits here with the measurement behind it.
enum IgemmFamily { IGEMM_TILE, IGEMM_RING, IGEMM_HALO };          // k_igemm2 / k_igemm2g, k_conv8p, k_conv3h
struct IgemmRoute {
    IgemmFamily family;
    int BM, BN, WM, WN, BK, LEAN;        // tile family: the template arguments of k_igemm2 (zero for the other two)
    dim3 grid, block;
    int lds, pieces_per_wave;            // dynamic LDS bytes; halo family: the second kernel argument
    int stats_rows;                      // rows of the [rows][2][N] partial-statistics buffer the launch writes when a.stats is set
};
// The four documented switches of the two specialised kernels, read per call (the parity tests lower the tile counts to reach small shapes)
struct IgemmSwitches { bool conv8p, conv3h; long conv8p_min_tiles, conv3h_min_tiles; };
static inline IgemmSwitches igemm_switches() {
    const char *on8 = getenv("PK_CONV8P"), *mt8 = getenv("PK_CONV8P_MIN_TILES"), *on3 = getenv("PK_CONV3H"), *mt3 = getenv("PK_CONV3H_MIN_TILES");
    // k_conv8p, one workgroup per CU: below one full round of 256 tiles the 128 x 128 tiles of k_igemm2 spread the work over more CUs.
    // k_conv3h: 16x12 x 64 samples = 126 tiles run 11.4 us against 15.3 us on k_igemm2.
    return IgemmSwitches{!on8 || atoi(on8) != 0, !on3 || atoi(on3) != 0, mt8 ? atol(mt8) : 256, mt3 ? atol(mt3) : 96};
}
static inline int conv3h_pieces_per_wave(int Ws, int Cin) {
    const int R = 128 + 2 * (Ws + 3), RP = 1024 / (Cin * 2);
    return ((R + RP - 1) / RP + 3) / 4;
}
static inline long conv3h_tiles(const IgemmArgs& a) {          // 128-position tiles of the zero-bordered images
    const long Mp = (long)(a.M / (a.Hs * a.Ws)) * (a.Hs + 2) * (a.Ws + 2);
    return Mp < (1 << 24) ? (Mp + 127) / 128 : -1;
}
// what both specialised kernels ask of a launch: a stride-1 same-size convolution with the plain or the scale / shift (/ ReLU) epilogue
static inline bool conv_plain(const IgemmArgs& a) {
    return a.Ho > 0 && a.stride == 1 && !a.dilated && a.Hs == a.Ho && a.Ws == a.Wo && a.out_mode == 0 && (!a.bias || a.col_scale) && !a.res_scale &&
           !a.a_rowmap && !a.o_rowmap && !a.preact && !a.gelu_of && (a.act == 0 || (a.act == 3 && !a.stats)) && a.ldo == a.N &&
           !(a.col_scale && (a.stats || !a.bias || (((uintptr_t)a.col_scale | (uintptr_t)a.bias) & 15)));
}
static inline bool conv3h_takes(const IgemmArgs& a, const IgemmSwitches& sw) {
    if (!(sw.conv3h && conv_plain(a) && a.T == 9 && (a.Cin == 32 || a.Cin == 64) && (a.N == 32 || a.N == 64) && !(a.res && a.stats))) return false;
    const int pp = conv3h_pieces_per_wave(a.Ws, a.Cin);
    if (pp < 3 || pp > 11) return false;                       // the counted vmcnt waits are compiled for 3 .. 11 pieces per wave (W <= ~96 at 64 channels)
    const long ntiles = conv3h_tiles(a);
    return ntiles >= 0 && ntiles >= sw.conv3h_min_tiles;
}
static inline bool conv8p_takes(const IgemmArgs& a, const IgemmSwitches& sw) {
    return sw.conv8p && conv_plain(a) && (a.T == 9 || a.T == 1) && (a.N % 256) == 0 && (a.Cin % 32) == 0 && a.T * a.Cin >= 576 && !a.res &&
           (((uintptr_t)a.out) & 15) == 0 && (long)((a.M + 255) / 256) * (a.N / 256) >= sw.conv8p_min_tiles;
}
// Fills the launcher-owned fields of `a` and returns the route.  Pure: no HIP call, no environment; pointers are tested for null and alignment only.
static IgemmRoute igemm_route(IgemmArgs& a, int cus, const IgemmSwitches& sw) {
    a.vec8 = (a.ldo % 8) == 0 && ((((uintptr_t)a.out | (uintptr_t)a.res | (uintptr_t)a.preact | (uintptr_t)a.gelu_of) & 15) == 0);
    a.xcd_remap = 1;
    a.chunk_major = a.T == 9 && a.N <= 32 && a.Cin >= 128 && (a.Cin % 64) == 0 && !a.dilated;      // (the dilated walk has its own tap list)
    a.dil_group = a.dilated && a.T == 9 && a.out_mode == 0 && !a.stats && !a.o_rowmap && !a.res_scale;
    IgemmRoute r{};
    r.stats_rows = (a.M + STAT_ROWS - 1) / STAT_ROWS;          // one row per 128 output pixels, whatever the tile
    if (conv3h_takes(a, sw)) {
        // persistent workgroups, two per CU (the 64 -> 64 variant holds 232 VGPRs); one statistics row per workgroup and position half
        const long ntiles = conv3h_tiles(a);
        const int grid = (int)(ntiles < 2L * cus ? ntiles : 2L * cus);
        r.family = IGEMM_HALO; r.grid = dim3((unsigned)grid); r.block = dim3(256); r.stats_rows = 2 * grid;
        r.pieces_per_wave = conv3h_pieces_per_wave(a.Ws, a.Cin); r.lds = 2 * r.pieces_per_wave * 4096;
        return r;
    }
    if (conv8p_takes(a, sw)) {
        r.family = IGEMM_RING; r.grid = dim3((unsigned)(((a.M + 255) / 256) * (a.N / 256))); r.block = dim3(512);
        return r;
    }
    r.family = IGEMM_TILE; r.block = dim3(256);
    // plain launches (no dilated gather) take the LEAN = 3 instantiation of a tile, the stride-2 data gradients LEAN = 4: see the kernel's first lines
    const int plain = a.dilated ? 4 : 3;
    // Deep contractions with wide outputs (the 3x3 convs of the head: K = 2304, N = 128/256): 256 x 128 workgroup tile, 128 x 64
    // per wave -- a third less LDS traffic per MFMA than the 64 x 64 wave tile, which is what bounds those kernels.
    // (needs >= 1024 workgroups: with 768 -- N = 128 at M = 196 608 -- the second round of workgroups is half empty and the
    // kernel is slower than the 128 x 128 tile.  Measured at N = 256: fwd 361 -> 334 us, dgrad 306 -> 285 us.)
    if ((a.N % 128) == 0 && a.T * a.Cin >= 576 && (a.Cin % 32) == 0 && (long)((a.M + 255) / 256) * (a.N / 128) >= 1024) {
        r.BM = 256; r.BN = 128; r.WM = 2; r.WN = 2; r.BK = 32; r.LEAN = plain;
        r.grid = dim3((a.M + 255) / 256, a.N / 128);
        return r;
    }
    const unsigned gm = (unsigned)((a.M + 127) / 128);
    // deeper K-chunks when the channel count allows full 64-wide tiles -- except for contractions of <= 128 (one or two steps): the BK = 32
    // variants hold half the LDS and run 4-7 waves per SIMD instead of 3, which is what an output-bound launch needs (1x1 64 -> 256 @64x48
    // data gradient 48.5 -> 37 us)
    constexpr int shallow32 = 128;
    const bool k64 = (a.Cin % 64) == 0 && !(a.T * a.Cin <= shallow32);
    // the lean instantiations (1: plain linear, 2: linear with preact / gelu_of / GELU) exist for the 128 x 32 and 128 x 64 tiles at BK = 64
    const bool lean_any = a.T == 1 && a.Ho == 0 && !a.stats && a.act <= 1 && a.out_mode == 0 && a.vec8 && k64 && (a.N % 8) == 0;
    const bool lean = lean_any && !a.preact && !a.gelu_of && a.act == 0;
    const int lean_or_plain = lean ? 1 : (lean_any ? 2 : plain);
    // Shallow contractions (K = T*Cin <= 256: the token-MLP / qkv GEMMs) are bound by their output traffic, not MFMA:
    // 128x64 tiles need half the accumulators (4 waves/SIMD instead of 2) and hide the epilogue's memory latency better
    // (measured 24 vs 32 us for qkv K=32 N=96, 43 vs 51 us for fc1+GELU K=32 N=128, 17 vs 21 us for K=128 N=512).
    // Few pixel rows (low-resolution branches: 24 .. 96 row tiles): a 128-wide N tile leaves most of the 256 CUs idle, so take
    // the widest N tile that still gives >= 512 workgroups (they are latency-bound, not MFMA-bound, at that size).
    // (128 x 64 tiles for the large convs were measured too: head conv 421 us instead of 361 us.)
    const bool small_m = a.N > 64 && (long)gm * ((a.N + 127) / 128) < 512;
    // (shallow convs with statistics too: 1x1 64 -> 256 forward 57 -> 47.6 us)
    if (small_m && (long)gm * ((a.N + 63) / 64) < 512 && !a.stats) { r.BN = 32; r.LEAN = lean_or_plain; }
    else if (a.N > 64 && (a.T * a.Cin <= 256 || small_m) && (!a.stats || a.T * a.Cin <= 256)) { r.BN = 64; r.LEAN = lean_or_plain; }
    else if (a.N > 64) { r.BN = 128; r.LEAN = plain; }
    else if (a.N > 32) { r.BN = 64; r.LEAN = lean_or_plain; }
    else { r.BN = 32; r.LEAN = plain; }
    r.BM = 128; r.WM = r.BN == 128 ? 2 : 4; r.WN = r.BN == 128 ? 2 : 1; r.BK = k64 ? 64 : 32;
    r.grid = dim3(gm, (a.N + r.BN - 1) / r.BN);
    return r;
}

// Every instantiation of the tile family, named once: X(BM, BN, WM, WN, BK, LEAN).
#define IGEMM_TILES(X)                                                                                                                  \
    X(256, 128, 2, 2, 32, 3) X(256, 128, 2, 2, 32, 4)                                                                                  \
    X(128, 128, 2, 2, 64, 3) X(128, 128, 2, 2, 64, 4) X(128, 128, 2, 2, 32, 3) X(128, 128, 2, 2, 32, 4)                                \
    X(128, 64, 4, 1, 64, 1) X(128, 64, 4, 1, 64, 2) X(128, 64, 4, 1, 64, 3) X(128, 64, 4, 1, 64, 4) X(128, 64, 4, 1, 32, 3) X(128, 64, 4, 1, 32, 4) \
    X(128, 32, 4, 1, 64, 1) X(128, 32, 4, 1, 64, 2) X(128, 32, 4, 1, 64, 3) X(128, 32, 4, 1, 64, 4) X(128, 32, 4, 1, 32, 3) X(128, 32, 4, 1, 32, 4)
// ... and of the grouped form (pk_conv2d_group: the 128 x 32 tile only)
#define IGEMM_GROUP_TILES(X) X(128, 32, 4, 1, 64, 3) X(128, 32, 4, 1, 64, 4) X(128, 32, 4, 1, 32, 3) X(128, 32, 4, 1, 32, 4)
static constexpr int igemm_tile_key(int BM, int BN, int BK, int LEAN) { return ((BM * 1000 + BN) * 100 + BK) * 10 + LEAN; }      // (WM, WN follow from BN)
#define IGEMM_TILE_SWITCH(KERN, TILES)                                                                           \
    switch (igemm_tile_key(r.BM, r.BN, r.BK, r.LEAN)) {                                                          \
        TILES(IGEMM_TILE_CASE_##KERN)                                                                            \
        default: pk_set_error("%s: no " #KERN " instantiation for the tile %d x %d, BK %d, LEAN %d", who, r.BM, r.BN, r.BK, r.LEAN); return PK_ERR_UNSUPPORTED; \
    }
#define IGEMM_TILE_CASE_k_igemm2(BM_, BN_, WM_, WN_, BK_, LEAN_) \
    case igemm_tile_key(BM_, BN_, BK_, LEAN_): hipLaunchKernelGGL((k_igemm2<BM_, BN_, WM_, WN_, BK_, LEAN_>), r.grid, r.block, r.lds, st, a); break;
#define IGEMM_TILE_CASE_k_igemm2g(BM_, BN_, WM_, WN_, BK_, LEAN_) \
    case igemm_tile_key(BM_, BN_, BK_, LEAN_): hipLaunchKernelGGL((k_igemm2g<BM_, BN_, WM_, WN_, BK_, LEAN_>), r.grid, r.block, r.lds, st, g); break;
// the halo kernel asks for its largest LDS size once per instantiation
#define CONV3H_CASE(CI, CO)                                                                                                                   \
    case CI * 100 + CO: {                                                                                                                     \
        static bool attr_done = false;                                                                                                        \
        const hipError_t e = attr_done ? hipSuccess : hipFuncSetAttribute((const void*)k_conv3h<CI, CO>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 11 * 4096); \
        if (e != hipSuccess) return pk_set_error("%s: cannot raise the LDS limit of k_conv3h: %s", who, hipGetErrorString(e)), (int)e;        \
        attr_done = true;                                                                                                                     \
        hipLaunchKernelGGL((k_conv3h<CI, CO>), r.grid, r.block, r.lds, st, a, r.pieces_per_wave);                                             \
    } break;
static int igemm_launch(const IgemmArgs& a_in, hipStream_t st, const char* who) {
    IgemmArgs a = a_in;
    const IgemmRoute r = igemm_route(a, pk_cu_count(), igemm_switches());
    switch (r.family) {
    case IGEMM_HALO: switch (a.Cin * 100 + a.N) { CONV3H_CASE(64, 64) CONV3H_CASE(64, 32) CONV3H_CASE(32, 64) CONV3H_CASE(32, 32) } break;
    case IGEMM_RING: hipLaunchKernelGGL(k_conv8p, r.grid, r.block, r.lds, st, a); break;
    case IGEMM_TILE: IGEMM_TILE_SWITCH(k_igemm2, IGEMM_TILES) break;
    }
    return pk_launch_status(who);
}

// ================================================================================================ entry points
static int check_common(const char* who, const void* x, const void* w, const void* out, int M, int N, int Cin, int ldo, int out_mode) {
    PK_REQUIRE(x && w && out, "%s: null pointer", who);
    PK_REQUIRE(M > 0 && N > 0 && Cin > 0, "%s: bad sizes M=%d N=%d Cin=%d", who, M, N, Cin);
    PK_SUPPORTED((Cin & 7) == 0, "%s: Cin=%d must be a multiple of 8 (16-byte bf16 chunks)", who, Cin);
    PK_REQUIRE((((uintptr_t)x | (uintptr_t)w) & 15) == 0, "%s: x/w must be 16-byte aligned", who);
    if (out_mode != 2) {
        PK_REQUIRE(ldo >= N, "%s: ldo=%d < N=%d", who, ldo, N);
        PK_REQUIRE((ldo & 3) == 0 && ((uintptr_t)out & 15) == 0, "%s: output pitch must be a multiple of 4 and 16-byte aligned", who);
    }
    PK_REQUIRE((int64_t)M * (ldo > Cin ? ldo : Cin) < 0x3fffffffLL, "%s: tensor too large for 32-bit byte offsets", who);
    return PK_OK;
}
// Positive sizes, and an output size that matches the input, kernel and stride (or, for a stride-2 data gradient, the dilated input).
// `dilated_as`: the dilated_input of the first member of a group, which every member must share; -1 outside groups.
static int check_conv_geometry(const char* who, int B, int Hs, int Ws, int ksize, int stride, int dilated, int Ho, int Wo, int dilated_as = -1) {
    PK_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "%s: bad geometry", who);
    PK_REQUIRE(dilated_as < 0 || (dilated != 0) == (dilated_as != 0), "%s: members must agree on dilated_input", who);
    if (dilated) PK_REQUIRE(Ho <= 2 * Hs && Wo <= 2 * Ws && Ho >= 2 * Hs - 1 && Wo >= 2 * Ws - 1, "%s: dilated geometry %dx%d <- %dx%d", who, Ho, Wo, Hs, Ws);
    else PK_REQUIRE(Ho == (Hs + 2 * (ksize / 2) - ksize) / stride + 1 && Wo == (Ws + 2 * (ksize / 2) - ksize) / stride + 1,
                    "%s: output %dx%d does not match input %dx%d k=%d s=%d", who, Ho, Wo, Hs, Ws, ksize, stride);
    return PK_OK;
}
static int check_conv_extent(const char* who, int B, int Hs, int Ws, int Cin, int Cout, int ksize) {
    PK_REQUIRE((int64_t)B * Hs * Ws * Cin < 0x3fffffffLL && (int64_t)Cout * ksize * ksize * Cin < 0x3fffffffLL, "%s: input too large for 32-bit byte offsets", who);
    return PK_OK;
}
// the argument block of a convolution, epilogue options left at "none"
static IgemmArgs conv_args(const void* x, const void* w, void* out, int B, int Hs, int Ws, int Cin, int Cout, int ksize, int stride, int dilated,
                           int Ho, int Wo) {
    IgemmArgs a{};
    a.x = (const uint16_t*)x; a.w = (const uint16_t*)w; a.out = out;
    a.M = B * Ho * Wo; a.N = Cout; a.Cin = Cin; a.T = ksize * ksize; a.Hs = Hs; a.Ws = Ws; a.Ho = Ho; a.Wo = Wo;
    a.stride = stride; a.pad = ksize / 2; a.dilated = dilated; a.ldo = Cout; a.rows_per_sample = Ho * Wo;
    return a;
}

extern "C" int pk_conv2d_nhwc(const void* x, const void* w_packed, void* out, float* stats_partial, const float* bias,
                              int B, int Hs, int Ws, int Cin, int Cout, int ksize, int stride, int dilated_input, int Ho,
                              int Wo, int act, int out_mode, const void* addend, void* stream) {
    const char* who = "pk_conv2d_nhwc";
    int rc = check_common(who, x, w_packed, out, B * Ho * Wo, Cout, Cin, Cout, out_mode);
    if (rc) return rc;
    PK_REQUIRE(ksize == 1 || ksize == 3, "pk_conv2d_nhwc: ksize %d", ksize);
    PK_REQUIRE(stride == 1 || (stride == 2 && !dilated_input), "pk_conv2d_nhwc: stride %d", stride);
    if ((rc = check_conv_geometry(who, B, Hs, Ws, ksize, stride, dilated_input, Ho, Wo))) return rc;
    PK_REQUIRE(out_mode >= 0 && out_mode <= 2 && act >= 0 && act <= 2, "pk_conv2d_nhwc: bad mode");
    if ((rc = check_conv_extent(who, B, Hs, Ws, Cin, Cout, ksize))) return rc;
    PK_REQUIRE(out_mode == 2 || (Cout & 3) == 0, "pk_conv2d_nhwc: Cout=%d must be a multiple of 4 for row-major output", Cout);
    IgemmArgs a = conv_args(x, w_packed, out, B, Hs, Ws, Cin, Cout, ksize, stride, dilated_input, Ho, Wo);
    a.bias = bias; a.stats = stats_partial; a.act = act; a.out_mode = out_mode;
    PK_REQUIRE(!addend || (out_mode == 0 && !stats_partial), "pk_conv2d_nhwc: an addend needs the bf16 row-major output and no statistics");
    a.res = (const uint16_t*)addend;          // out = conv(x) + addend (same shape, bf16): the skip connection's gradient in a data-gradient launch
    return igemm_launch(a, (hipStream_t)stream, who);
}

// conv -> eval-mode BatchNorm (-> + residual) (-> ReLU) in ONE launch: y = relu?(col_scale[n] * conv(x)[., n] + col_shift[n] + residual).
// Inference only (the scale / shift are the constants gamma * rsqrt(running_var + eps), beta - running_mean * that); stride 1 or 2.
extern "C" int pk_conv2d_affine_nhwc(const void* x, const void* w_packed, void* out, const float* col_scale, const float* col_shift,
                                     const void* residual, int relu, int B, int Hs, int Ws, int Cin, int Cout, int ksize, int stride, int Ho,
                                     int Wo, void* stream) {
    const char* who = "pk_conv2d_affine_nhwc";
    int rc = check_common(who, x, w_packed, out, B * Ho * Wo, Cout, Cin, Cout, 0);
    if (rc) return rc;
    PK_REQUIRE(col_scale && col_shift, "pk_conv2d_affine_nhwc: null scale / shift");
    PK_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2), "pk_conv2d_affine_nhwc: ksize %d stride %d", ksize, stride);
    if ((rc = check_conv_geometry(who, B, Hs, Ws, ksize, stride, 0, Ho, Wo))) return rc;
    if ((rc = check_conv_extent(who, B, Hs, Ws, Cin, Cout, ksize))) return rc;
    PK_REQUIRE((Cout & 3) == 0, "pk_conv2d_affine_nhwc: Cout=%d must be a multiple of 4", Cout);
    IgemmArgs a = conv_args(x, w_packed, out, B, Hs, Ws, Cin, Cout, ksize, stride, 0, Ho, Wo);
    a.bias = col_shift; a.col_scale = col_scale; a.act = relu ? 3 : 0; a.res = (const uint16_t*)residual;
    return igemm_launch(a, (hipStream_t)stream, who);
}

// Grouped convolutions: n <= PK_GROUP_MAX members, each what one pk_conv2d_nhwc (train: bf16 output + statistics partials; data gradient:
// dilated_input / addend) or pk_conv2d_affine_nhwc (col_scale / bias / residual / relu) call would do, all on the 128 x 32 tile of k_igemm2
// (any Cout % 4 == 0; deep-K members share BK = 64 only when every member allows it).  Members must agree on `dilated_input`.
extern "C" int pk_conv2d_group(const PkConvDesc* d, int n, void* stream) {
    const char* who = "pk_conv2d_group";
    PK_REQUIRE(d && n > 0 && n <= PK_GROUP_MAX, "pk_conv2d_group: 1..%d members, got %d", PK_GROUP_MAX, n);
    IgemmGroup g{};
    bool k64 = true;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        const PkConvDesc& c = d[i];
        int rc = check_common(who, c.x, c.w, c.out, c.B * c.Ho * c.Wo, c.Cout, c.Cin, c.Cout, 0);
        if (rc) return rc;
        PK_REQUIRE(c.ksize == 1 || c.ksize == 3, "pk_conv2d_group: ksize %d", c.ksize);
        PK_REQUIRE(c.stride == 1 || (c.stride == 2 && !c.dilated_input), "pk_conv2d_group: stride %d", c.stride);
        if ((rc = check_conv_geometry(who, c.B, c.Hs, c.Ws, c.ksize, c.stride, c.dilated_input, c.Ho, c.Wo, d[0].dilated_input != 0))) return rc;
        if ((rc = check_conv_extent(who, c.B, c.Hs, c.Ws, c.Cin, c.Cout, c.ksize))) return rc;
        PK_REQUIRE((c.Cout & 3) == 0, "pk_conv2d_group: Cout=%d must be a multiple of 4", c.Cout);
        PK_REQUIRE(!(c.stats && (c.res || c.col_scale)), "pk_conv2d_group: statistics go with the plain bf16 output only");
        PK_REQUIRE(c.act == 0 || c.act == 3, "pk_conv2d_group: act %d (0 none, 3 ReLU after the residual)", c.act);
        IgemmArgs& a = g.a[i];
        a = conv_args(c.x, c.w, c.out, c.B, c.Hs, c.Ws, c.Cin, c.Cout, c.ksize, c.stride, c.dilated_input ? 1 : 0, c.Ho, c.Wo);
        a.bias = c.bias; a.col_scale = c.col_scale; a.stats = c.stats; a.res = (const uint16_t*)c.res; a.act = c.act;
        a.vec8 = (a.ldo % 8) == 0 && ((((uintptr_t)a.out | (uintptr_t)a.res) & 15) == 0);
        a.xcd_remap = 0;            // (the remap assumes a grid of its own; these tensors fit in any one L2)
        a.chunk_major = 0;
        a.dil_group = a.dilated && a.T == 9 && !a.stats;
        k64 = k64 && (a.Cin % 64) == 0 && a.T * a.Cin > 128;
        g.gy[i] = (a.N + 31) / 32;
        g.first[i] = total;
        total += ((a.M + 127) / 128) * g.gy[i];
    }
    g.first[n] = total;
    g.n = n;
    hipStream_t st = (hipStream_t)stream;
    IgemmRoute r{};          // the one tile of the grouped form; every member's workgroups in one grid
    r.BM = 128; r.BN = 32; r.WM = 4; r.WN = 1; r.BK = k64 ? 64 : 32; r.LEAN = d[0].dilated_input ? 4 : 3;
    r.grid = dim3((unsigned)total); r.block = dim3(256);
    IGEMM_TILE_SWITCH(k_igemm2g, IGEMM_GROUP_TILES)
    return pk_launch_status(who);
}

extern "C" int pk_conv_stats_tiles(int M) { return (M + STAT_ROWS - 1) / STAT_ROWS; }
// rows of the [rows][2][Cout] partial-statistics buffer that pk_conv2d_nhwc(bf16 output, statistics) writes for this geometry: the halo
// kernel emits one row per 64 PADDED positions, every other kernel one per 128 output pixels (pk_bn_finalize sums whatever it is given).
// The count is the route's, so it cannot disagree with the launch.
extern "C" int pk_conv_stats_rows(int B, int Hs, int Ws, int Cin, int Cout, int ksize, int stride, int Ho, int Wo) {
    static float statistics_wanted;          // the route reads pointers for null-ness and alignment only
    IgemmArgs a = conv_args(nullptr, nullptr, nullptr, B, Hs, Ws, Cin, Cout, ksize, stride, 0, Ho, Wo);
    a.stats = &statistics_wanted;
    return igemm_route(a, pk_cu_count(), igemm_switches()).stats_rows;
}

extern "C" int pk_linear_bf16(const void* x, const void* w, void* out, const float* bias, const void* residual,
                              const float* res_scale, const int32_t* a_rowmap, const int32_t* o_rowmap, void* preact_out,
                              const void* gelu_grad_of, int M, int N, int K, int rows_per_sample, int act, int out_fp32,
                              void* stream) {
    int rc = check_common("pk_linear_bf16", x, w, out, M, N, K, N, out_fp32 ? 1 : 0);
    if (rc) return rc;
    PK_REQUIRE((N & 3) == 0, "pk_linear_bf16: N=%d must be a multiple of 4", N);
    PK_REQUIRE(!res_scale || rows_per_sample > 0, "pk_linear_bf16: res_scale needs rows_per_sample");
    PK_REQUIRE(act >= 0 && act <= 1, "pk_linear_bf16: act %d", act);
    IgemmArgs a{};
    a.x = (const uint16_t*)x; a.w = (const uint16_t*)w; a.out = out; a.bias = bias; a.res = (const uint16_t*)residual;
    a.res_scale = res_scale; a.a_rowmap = a_rowmap; a.o_rowmap = o_rowmap;
    a.preact = (uint16_t*)preact_out; a.gelu_of = (const uint16_t*)gelu_grad_of;
    a.M = M; a.N = N; a.Cin = K; a.T = 1; a.Ho = 0; a.Wo = 0; a.ldo = N; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1;
    a.act = act; a.out_mode = out_fp32 ? 1 : 0;
    return igemm_launch(a, (hipStream_t)stream, "pk_linear_bf16");
}
