// BatchNorm (train) + ReLU + the 1x1 output convolution of a fusion-head branch (models/fusion_head.py: conv3x3 -> BN -> ReLU -> conv1x1 + bias
// -> 17 / 34 / 17 maps).  At 256x192, B = 64 the activated tensor t = relu(bn(raw)) and the output conv's data gradient dt are 196 608 rows x
// 256 channels of bf16 = 100.7 MB (T) each.  dt is a contraction of at most 40 deep of a tensor a sixth to a tenth of that size: it is never
// stored, both BatchNorm backward passes recompute the tile they need.  t is still written once (the output conv's weight gradient reads it:
// that sum stays k_wgrad4's, bit for bit), but the output conv no longer reads it back: it is contracted from the LDS tile it is written from.
//
//   stored route                                                   this unit
//   forward   k_bn_act reads raw (T), writes t (T), the 1x1 conv    k_bn_out1x1_fwd: reads raw (T), writes t (T), the maps and the ReLU bits
//             reads it (T)
//   backward  1x1 data gradient writes dt (T), k_bn_bwd_reduce     k_bn_out1x1_bwd<1>: reads raw (T), g, the bits; partial sums
//             reads dt, raw (2T), k_bn_bwd_apply reads dt, raw,    k_bn_out1x1_bwd<2>: reads raw (T), g, the bits; writes draw (T)
//             writes draw (3T)
//   9 T per full-width branch (+ k_wgrad4 reading t: T)            5 T per full-width branch (+ k_wgrad4 reading t: T)
//
// One row-panel body per mode.  A wave works on BLOCKS of 16 consecutive rows: the block's raw chunks (16 bytes = 8 channels) arrive by
// row-contiguous 16-byte loads (a wave-wide load covers 1 KB of whole rows), the per-element work is done in that layout, and the block's
// tile -- t in forward, dt in backward -- lives in the wave's LDS tile [16][C + 8] bf16 from which (or into which) the MFMA fragments go.
// The loads of the NEXT block are requested before the current one is computed.  256 threads = 4 waves per workgroup, persistent.
//
//   forward       t = bf16(relu(raw * scale + shift)) (k_bn_act's expression and its bit mask) -> global and LDS tile -> out = t Wf^T + bias
//                 (softplus): v_mfma_f32_16x16x32_bf16 with the weight as the A operand, k -> lane assignment and ascending 32-channel
//                 K-chunks as in k_igemm2, so `out` is bit for bit what pk_conv2d_nhwc computes from the stored t.  128-row tiles.
//   backward <1>  dt = bf16(g Wd^T) by the same instruction in the data-gradient launch's roles and K-chunks (g's and the weight's columns
//                 beyond up8(N) read as zeros) -> LDS tile -> masked by the ReLU bits, summed as k_bn_bwd_reduce sums: one WAVE per partial
//                 row of pk_bn_bwd_blocks(rows), lane rows = that kernel's row lanes, ascending, then the row lanes in order: the partial
//                 rows are pk_bn_bwd's on a stored dt bit for bit.
//   backward <2>  dt again, draw = gamma rstd (g - sum_g / M - xhat sum_gx / M) in k_bn_bwd_apply's expression (rows > 32 768) or
//                 k_bn_bwd_apply_fin's (below; the partial rows are then summed as that kernel sums them).  128-row tiles.
//
// Plan (hipcc -Rpass-analysis=kernel-resource-usage): no scratch in any instantiation; forward and <2>: __launch_bounds__(256, 2), two
// workgroups per CU; LDS = weight + 4 tiles (+ vectors): 50 688 / 59 136 bytes forward at C = 256 (N <= 32 / <= 48), 59 392 / 75 776 backward.
// <1>: pk_bn_bwd_blocks gives at most 1024 partial rows = 256 workgroups, one per CU, one wave per SIMD: __launch_bounds__(256, 1), the loads of
// two blocks ahead in flight (at C = 256 some of those values wait in AGPRs).
// No atomics, no grid-wide barrier, no spin-wait; every sum has a fixed order, two launches give identical bytes.
#include <stdlib.h>

#include "pk_rowops.h"

#define BO_ROWS 128
#define BO_GRID 512
#define BO_MIN_ROWS 32768        // from here pk_bn_train_fwd / pk_bn_bwd take their large-tensor form (pk_bn.hip)
#define BO_SMALL_ROWS 32768      // pk_bn_bwd's small-tensor rule (bn_bwd_small in pk_bn.hip): its apply kernel sums the partial rows itself

struct BnOutArgs {
    const uint4* raw;            // [rows][C] bf16
    const uint16_t* w;           // forward: packed forward weight [N][1][C]; backward: packed data-gradient weight [C][1][up8(N)]
    const uint16_t* g;           // backward: [rows][up8(N)] bf16, channels >= N zero
    const uint8_t* mask_in;      // backward: ReLU bits
    uint8_t* mask_out;           // forward
    const float* v0;             // forward: scale;  backward: mean
    const float* v1;             // forward: shift;  backward: rstd
    const float* gamma;          // backward <2>
    const float* sums;           // backward <2>: [2][C]
    const float* bias;           // forward: [N]
    float* out;                  // forward: fp32 NCHW planes [B][N][hw]
    uint4* t_out;                // forward: t [rows][C] bf16
    uint4* draw;                 // backward <2>
    float* part;                 // backward <1>: [nb][2][C]
    float inv_count;             // backward <2>
    int small;                   // backward <2>: k_bn_bwd_apply_fin's expression
    int64_t rows;
    int N, N8, hw, softplus;
    int nb, rpb;                 // backward <1>: partial rows and rows per partial row, the split of k_bn_bwd_reduce
};

template <int C>
struct BoGeom {
    static constexpr int CPR = C / 8;           // 16-byte chunks per row
    static constexpr int RPI = 64 / CPR;        // rows per wave-wide load
    static constexpr int NLD = 16 / RPI;        // loads per lane and block
    static constexpr int TP = C + 8;            // tile pitch in bf16 elements (16 bytes of padding per row)
    static constexpr int RL = 256 / CPR;        // row lanes of k_bn_bwd_reduce (8 at C = 256, 16 at C = 128): four per lane here
    static constexpr int TILE_BYTES = (16 * TP * 2 > RL * C * 4) ? 16 * TP * 2 : RL * C * 4;      // (<1> sums the row lanes through it)
};

__device__ __forceinline__ void bo_wave_sync() {          // the tiles are wave-private
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ================================================================================================ forward
template <int C, int NB>
__global__ void __launch_bounds__(256, 2) k_bn_out1x1_fwd(BnOutArgs p) {
    using G = BoGeom<C>;
    constexpr int CPR = G::CPR, RPI = G::RPI, NLD = G::NLD, TP = G::TP;
    extern __shared__ __attribute__((aligned(16))) unsigned char bo_smem[];
    uint16_t* sW = reinterpret_cast<uint16_t*>(bo_smem);                                   // [NB * 16][TP], rows >= N zero
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint16_t* tile = reinterpret_cast<uint16_t*>(bo_smem + NB * 16 * TP * 2) + wave * 16 * TP;
    const int frow = lane & 15, fkc = lane >> 4;
    const int lch = lane % CPR, lrw = lane / CPR;
    const int64_t rows = p.rows;
    const int ntiles = (int)((rows + BO_ROWS - 1) / BO_ROWS);
    auto block_base = [&](int it) -> int64_t {             // a wave's blocks: the two halves of its 32 rows of tile bid, bid + grid, ...
        const int64_t t = (int64_t)blockIdx.x + (int64_t)(it >> 1) * gridDim.x;
        return t < ntiles ? t * BO_ROWS + wave * 32 + (it & 1) * 16 : -1;
    };
    auto load_raw = [&](uint4 (&rv)[NLD], int64_t base) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int64_t row = base + i * RPI + lrw;
            rv[i] = make_uint4(0u, 0u, 0u, 0u);
            if (base >= 0 && row < rows) rv[i] = p.raw[(size_t)row * CPR + lch];
        }
    };
    uint4 rv[NLD], rn[NLD];
    int64_t base = block_base(0);
    load_raw(rv, base);
    for (int i = tid; i < NB * 16 * CPR; i += 256) {
        const int n = i / CPR, ch = i - n * CPR;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (n < p.N) v = reinterpret_cast<const u32x4*>(p.w)[(size_t)n * CPR + ch];
        *reinterpret_cast<u32x4*>(&sW[n * TP + ch * 8]) = v;
    }
    float sc[8], sh[8], bs[NB][4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = p.v0[lch * 8 + j];
        sh[j] = p.v1[lch * 8 + j];
    }
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = a * 16 + fkc * 4 + r;
            bs[a][r] = n < p.N ? p.bias[n] : 0.f;
        }
    __syncthreads();
    for (int it = 0; base >= 0; ++it) {
        const int64_t nbase = block_base(it + 1);
        load_raw(rn, nbase);
        bo_wave_sync();                                    // the previous block's fragments have been read
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int rl = i * RPI + lrw;
            const int64_t row = base + rl;
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
            if (row < rows) {
                float v[8];
                unpack8(rv[i], v);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j] * sc[j] + sh[j], 0.f);      // k_bn_act's expression
                o = pack8(v);
                p.t_out[(size_t)row * CPR + lch] = o;
                p.mask_out[(size_t)row * CPR + lch] = (uint8_t)pos_mask8(o);
            }
            *reinterpret_cast<uint4*>(&tile[rl * TP + lch * 8]) = o;
        }
        bo_wave_sync();
        f32x4 acc[NB];
#pragma unroll
        for (int a = 0; a < NB; ++a) acc[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < C / 32; ++ks) {
            const bf16x8 tf = *reinterpret_cast<const bf16x8*>(&tile[frow * TP + (ks * 4 + fkc) * 8]);
#pragma unroll
            for (int a = 0; a < NB; ++a) {
                const bf16x8 wf = *reinterpret_cast<const bf16x8*>(&sW[(a * 16 + frow) * TP + (ks * 4 + fkc) * 8]);
                acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, tf, acc[a], 0, 0, 0);
            }
        }
        const int64_t row = base + frow;
        if (row < rows) {
            const int bb = (int)(row / p.hw), pix = (int)(row - (int64_t)bb * p.hw);
            float* o = p.out + (size_t)bb * p.N * p.hw + pix;
#pragma unroll
            for (int a = 0; a < NB; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = a * 16 + fkc * 4 + r;
                    if (n < p.N) {
                        float v = acc[a][r] + bs[a][r];
                        if (p.softplus) v = softplus_(v);
                        o[(size_t)n * p.hw] = v;
                    }
                }
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) rv[i] = rn[i];
        base = nbase;
    }
}

// ================================================================================================ backward
// MODE 1: reduce, MODE 2: apply.  KP: the contraction depth in whole K-chunks (up8(N) rounded up to 32).
template <int MODE, int C, int KP>
__global__ void __launch_bounds__(256, MODE == 1 ? 1 : 2) k_bn_out1x1_bwd(BnOutArgs p) {
    using G = BoGeom<C>;
    constexpr int CPR = G::CPR, RPI = G::RPI, NLD = G::NLD, TP = G::TP, RL = G::RL;
    constexpr int WP = KP + 8, KS = KP / 32;               // pitch of the weight tile; K-chunks
    extern __shared__ __attribute__((aligned(16))) unsigned char bo_smem[];
    uint16_t* sWd = reinterpret_cast<uint16_t*>(bo_smem);                                  // [C][WP], columns >= up8(N) zero
    float* sVec = reinterpret_cast<float*>(bo_smem + C * WP * 2);                          // [5][C]
    unsigned char* tiles = bo_smem + C * WP * 2 + 5 * C * 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint16_t* tile = reinterpret_cast<uint16_t*>(tiles + wave * G::TILE_BYTES);
    const int frow = lane & 15, fkc = lane >> 4;
    const int lch = lane % CPR, lrw = lane / CPR;
    const int64_t rows = p.rows;
    const int ntiles = (int)((rows + BO_ROWS - 1) / BO_ROWS);
    // MODE 1: round q gives wave w the partial row (bid + q grid) 4 + w, every partial row is bpu blocks long
    const int bpu = (p.rpb + 15) / 16;
    const int total_it = MODE == 1 ? ((p.nb + 4 * (int)gridDim.x - 1) / (4 * (int)gridDim.x)) * bpu : 0;
    auto position = [&](int it, int& unit, int64_t& base, int64_t& end) {
        base = end = 0;
        unit = -1;
        if (MODE == 1) {
            const int q = it / bpu, k = it - q * bpu;
            const int u = ((int)blockIdx.x + q * (int)gridDim.x) * 4 + wave;
            if (it < total_it && u < p.nb) {
                unit = u;
                base = (int64_t)u * p.rpb + 16 * k;
                end = min(rows, (int64_t)(u + 1) * p.rpb);
            }
        } else {
            const int64_t t = (int64_t)blockIdx.x + (int64_t)(it >> 1) * gridDim.x;
            if (t < ntiles) {
                unit = 0;
                base = t * BO_ROWS + wave * 32 + (it & 1) * 16;
                end = rows;
            }
        }
    };
    struct Block {
        uint4 rv[NLD];
        uint32_t mv[NLD];
        bf16x8 gf[KS];
    };
    auto load_block = [&](Block& b, int64_t base, int64_t end) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int64_t row = base + i * RPI + lrw;
            b.rv[i] = make_uint4(0u, 0u, 0u, 0u);
            b.mv[i] = 0u;
            if (row < end) {
                b.rv[i] = p.raw[(size_t)row * CPR + lch];
                b.mv[i] = p.mask_in[(size_t)row * CPR + lch];
            }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int64_t row = base + frow;
            b.gf[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (row < end && (ks * 4 + fkc) * 8 < p.N8) b.gf[ks] = *reinterpret_cast<const bf16x8*>(p.g + (size_t)row * p.N8 + (ks * 4 + fkc) * 8);
        }
    };
    // MODE 1 runs one wave per SIMD (1024 partial rows at most) on a chain of a dozen blocks: it keeps the loads of TWO blocks ahead in flight
    Block cur, nxt, nx2;
    int unit, nunit;
    int64_t base, end, nbase, nend;
    position(0, unit, base, end);
    load_block(cur, base, end);
    position(1, nunit, nbase, nend);
    if (MODE == 1) load_block(nxt, nbase, nend);
    // ---- once per workgroup: the weight (zero beyond its up8(N) columns) and the per-channel vectors
    {
        const int wch = p.N8 / 8;
        for (int i = tid; i < C * (KP / 8); i += 256) {
            const int c = i / (KP / 8), ch = i - c * (KP / 8);
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ch < wch) v = reinterpret_cast<const u32x4*>(p.w)[(size_t)c * wch + ch];
            *reinterpret_cast<u32x4*>(&sWd[c * WP + ch * 8]) = v;
        }
        for (int c = tid; c < C; c += 256) {
            sVec[c] = p.v0[c];
            sVec[C + c] = p.v1[c];
            if (MODE == 2) {
                sVec[2 * C + c] = p.gamma[c];
                sVec[3 * C + c] = p.sums[c];
                sVec[4 * C + c] = p.sums[C + c];
            }
        }
    }
    float s1[4][8], s2[4][8];                              // MODE 1: the lane's four row lanes of the current partial row
    if (MODE == 1) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) s1[s][j] = s2[s][j] = 0.f;
    }
    __syncthreads();
    for (int it = 0; MODE == 1 ? it < total_it : unit >= 0; ++it) {
        int n2unit = -1;
        int64_t n2base = 0, n2end = 0;
        if (MODE == 1) {
            position(it + 2, n2unit, n2base, n2end);
            load_block(nx2, n2base, n2end);
        } else {
            load_block(nxt, nbase, nend);
        }
        // ---- (1) dt = bf16(g Wd^T): the data-gradient launch's MFMA (weight rows = channels as the A operand), 64 channels at a time
        bo_wave_sync();                                    // the previous block's tile has been read
#pragma unroll
        for (int cg = 0; cg < C / 64; ++cg) {
            f32x4 acc[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(&sWd[(cg * 64 + a * 16 + frow) * WP + (ks * 4 + fkc) * 8]);
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, cur.gf[ks], acc[a], 0, 0, 0);
                }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                // (+ 0: the stored route's epilogue adds its absent bias, which turns a -0 accumulator into +0 before the bf16 store)
                const u32x2 d = {pack_bf16x2(acc[a][0] + 0.f, acc[a][1] + 0.f), pack_bf16x2(acc[a][2] + 0.f, acc[a][3] + 0.f)};
                *reinterpret_cast<u32x2*>(&tile[frow * TP + cg * 64 + a * 16 + fkc * 4]) = d;
            }
        }
        bo_wave_sync();
        // ---- (2) per 8-channel row chunk: mask, sums or draw
        {
            float mu[8], rs[8], va[8], vb[8], vc[8];
            {
                const int c0 = lch * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    mu[j] = sVec[c0 + j];
                    rs[j] = sVec[C + c0 + j];
                    va[j] = MODE == 2 ? sVec[2 * C + c0 + j] : 0.f;
                    vb[j] = MODE == 2 ? sVec[3 * C + c0 + j] : 0.f;
                    vc[j] = MODE == 2 ? sVec[4 * C + c0 + j] : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int rl = i * RPI + lrw;
                const int64_t row = base + rl;
                const uint16_t* cell = &tile[rl * TP + lch * 8];
                if (row >= end) continue;
                float g[8], xr[8];
                unpack8(*reinterpret_cast<const uint4*>(cell), g);
                unpack8(cur.rv[i], xr);
                const uint32_t mb = cur.mv[i];
                if (MODE == 1) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float gg = ((mb >> j) & 1u) ? g[j] : 0.f;
                        s1[i & 3][j] += gg;
                        s2[i & 3][j] += gg * (xr[j] - mu[j]) * rs[j];
                    }
                } else {
                    float o[8];
                    if (p.small) {                         // k_bn_bwd_apply_fin
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float gg = ((mb >> j) & 1u) ? g[j] : 0.f;
                            const float gm = va[j] * rs[j], t1 = vb[j] * p.inv_count, t2 = vc[j] * p.inv_count;
                            const float xh = (xr[j] - mu[j]) * rs[j];
                            o[j] = gm * (gg - t1 - xh * t2);
                        }
                    } else {                               // k_bn_bwd_apply
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float gg = ((mb >> j) & 1u) ? g[j] : 0.f;
                            const float xh = (xr[j] - mu[j]) * rs[j];
                            o[j] = va[j] * rs[j] * (gg - vb[j] * p.inv_count - xh * vc[j] * p.inv_count);
                        }
                    }
                    p.draw[(size_t)row * CPR + lch] = pack8(o);
                }
            }
        }
        if (MODE == 1) {
            // ---- the partial row is complete: its row lanes in order (k_bn_bwd_reduce's last stage), through the wave's tile as [RL][C] floats
            if (unit >= 0 && it - (it / bpu) * bpu == bpu - 1) {
                float* stage = reinterpret_cast<float*>(tile);
                float* dst = p.part + (size_t)unit * 2 * C;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    bo_wave_sync();
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            stage[(s * RPI + lrw) * C + lch * 8 + j] = h ? s2[s][j] : s1[s][j];
                            if (h) s1[s][j] = s2[s][j] = 0.f;
                        }
                    bo_wave_sync();
#pragma unroll
                    for (int q = 0; q < C / 64; ++q) {
                        float a = 0.f;
#pragma unroll
                        for (int k = 0; k < RL; ++k) a += stage[k * C + q * 64 + lane];
                        dst[h * C + q * 64 + lane] = a;
                    }
                }
                bo_wave_sync();
            }
        }
        cur = nxt;
        unit = nunit;
        base = nbase;
        end = nend;
        if (MODE == 1) {
            nxt = nx2;
            nunit = n2unit;
            nbase = n2base;
            nend = n2end;
        } else {
            position(it + 2, nunit, nbase, nend);
        }
    }
}

// pk_bn_bwd's small-tensor form sums the partial rows inside its apply kernel (bn_bwd_apply_fin_body): 8 lanes per channel over the rows in
// double, then the lanes in order, rounded to fp32 once.  The same sums for backward <2>'s `small` expression, and dbeta / dgamma.
__global__ void __launch_bounds__(256) k_bn_out1x1_sum_small(const float* __restrict__ part, int nb, int C, float* __restrict__ sums,
                                                             float* __restrict__ dbeta, float* __restrict__ dgamma) {
    __shared__ double sh1[8][32], sh2[8][32];
    const int c0 = (int)blockIdx.x * 32;
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5, c = c0 + cl;
    double a = 0.0, b = 0.0;
    if (c < C)
        for (int t = pl; t < nb; t += 8) {
            a += (double)part[(size_t)t * 2 * C + c];
            b += (double)part[(size_t)t * 2 * C + C + c];
        }
    sh1[pl][cl] = a;
    sh2[pl][cl] = b;
    __syncthreads();
    if (threadIdx.x < 32 && c < C) {
        a = b = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a += sh1[k][cl];
            b += sh2[k][cl];
        }
        sums[c] = (float)a;
        sums[C + c] = (float)b;
        dbeta[c] = (float)a;
        dgamma[c] = (float)b;
    }
}

// ================================================================================================ routing and entries
// Three per-call switches, after the PK_CONV1X1_BN* precedent: PK_BN_OUT1X1=0 turns the route off, PK_BN_OUT1X1_MIN_ROWS sets the row
// threshold (the tests reach small and ragged shapes with it), PK_BN_OUT1X1_MAX_GRID caps the workgroups of a launch (one workgroup then
// walks several tiles and partial rows).
static inline int bo_grid(int64_t want) {
    const char* cap = getenv("PK_BN_OUT1X1_MAX_GRID");
    int64_t lim = BO_GRID;
    if (cap && atoi(cap) >= 1 && atoi(cap) < BO_GRID) lim = atoi(cap);
    if (want > lim) want = lim;
    return (int)(want < 1 ? 1 : want);
}
static inline bool bo_shape_ok(int64_t rows, int C, int N) { return rows > 0 && rows < (1 << 30) && (C == 256 || C == 128) && N >= 1 && N <= 48; }
extern "C" int pk_bn_out1x1_supported(int64_t rows, int C, int N) {
    const char *on = getenv("PK_BN_OUT1X1"), *mr = getenv("PK_BN_OUT1X1_MIN_ROWS");
    if (on && on[0] == '0') return 0;
    int64_t min_rows = BO_MIN_ROWS;
    if (mr && atoll(mr) >= 1) min_rows = atoll(mr);
    return (bo_shape_ok(rows, C, N) && rows >= min_rows) ? 1 : 0;
}
static inline bool bo_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}
#define BO_CHECK_SHAPE(who)                                                     \
    PK_REQUIRE(rows > 0 && rows < (1 << 30) && N > 0, who ": bad sizes");       \
    PK_SUPPORTED(bo_shape_ok(rows, C, N), who ": built for C = 128 / 256 channels and N <= 48 outputs (got %d -> %d)", C, N)

// (`attr_set`: one flag per kernel instantiation, owned by the caller)
static int bo_launch(void (*kernel)(BnOutArgs), bool& attr_set, int grid, int lds, const BnOutArgs& a, hipStream_t st, const char* who) {
    // may exceed 64 KB of LDS: asked for once per kernel (during the eager warm-up steps, not inside a graph capture)
    const hipError_t e = attr_set ? hipSuccess : hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return pk_set_error("%s: cannot reserve %d bytes of LDS: %s", who, lds, hipGetErrorString(e)), (int)e;
    attr_set = true;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), lds, st, a);
    return pk_launch_status(who);
}
template <int C, int NB>
static int bo_fwd(const BnOutArgs& a, hipStream_t st, const char* who) {
    static bool attr_set = false;
    const int lds = NB * 16 * BoGeom<C>::TP * 2 + 4 * 16 * BoGeom<C>::TP * 2;
    return bo_launch(k_bn_out1x1_fwd<C, NB>, attr_set, bo_grid((a.rows + BO_ROWS - 1) / BO_ROWS), lds, a, st, who);
}
template <int MODE, int C, int KP>
static int bo_bwd(const BnOutArgs& a, hipStream_t st, const char* who) {
    const int lds = C * (KP + 8) * 2 + 5 * C * 4 + 4 * BoGeom<C>::TILE_BYTES;
    const int grid = MODE == 1 ? bo_grid((a.nb + 3) / 4) : bo_grid((a.rows + BO_ROWS - 1) / BO_ROWS);
    static bool attr_set = false;
    return bo_launch(k_bn_out1x1_bwd<MODE, C, KP>, attr_set, grid, lds, a, st, who);
}
template <int MODE>
static int bo_bwd_any(const BnOutArgs& a, int C, hipStream_t st, const char* who) {
    if (C == 256) return a.N <= 32 ? bo_bwd<MODE, 256, 32>(a, st, who) : bo_bwd<MODE, 256, 64>(a, st, who);
    return a.N <= 32 ? bo_bwd<MODE, 128, 32>(a, st, who) : bo_bwd<MODE, 128, 64>(a, st, who);
}

// t = relu(raw * scale + shift) and relu_mask as k_bn_act writes them, out [B][N][hw] fp32 = conv1x1(t) + bias (softplus); rows = B hw.
extern "C" int pk_bn_out1x1_fwd(const void* raw, const float* scale, const float* shift, const void* w_fwd, const float* bias, void* t, float* out,
                                uint8_t* relu_mask, int64_t rows, int C, int N, int hw, int softplus, void* stream) {
    PK_REQUIRE(raw && scale && shift && w_fwd && bias && t && out && relu_mask, "pk_bn_out1x1_fwd: null pointer");
    BO_CHECK_SHAPE("pk_bn_out1x1_fwd");
    PK_REQUIRE(hw > 0 && rows % hw == 0, "pk_bn_out1x1_fwd: rows = %lld is no multiple of the plane size %d", (long long)rows, hw);
    PK_REQUIRE(bo_aligned(raw, w_fwd, t), "pk_bn_out1x1_fwd: raw, t and the weight must be 16-byte aligned");
    BnOutArgs a{};
    a.raw = (const uint4*)raw;
    a.w = (const uint16_t*)w_fwd;
    a.v0 = scale;
    a.v1 = shift;
    a.bias = bias;
    a.out = out;
    a.t_out = (uint4*)t;
    a.mask_out = relu_mask;
    a.rows = rows;
    a.N = N;
    a.hw = hw;
    a.softplus = softplus ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const char* who = "pk_bn_out1x1_fwd";
    if (C == 256) return N <= 32 ? bo_fwd<256, 2>(a, st, who) : bo_fwd<256, 3>(a, st, who);
    return N <= 32 ? bo_fwd<128, 2>(a, st, who) : bo_fwd<128, 3>(a, st, who);
}

// pk_bn_bwd (training mode, ReLU bits) of dt = conv1x1 data gradient of g, dt never stored: reduce, the fixed-order sum of the partial rows
// (sums = [sum g | sum g xhat], the same values to dbeta / dgamma), apply.
//   g: [rows][up8(N)] bf16, channels >= N zero;  w_dgrad: the packed data-gradient weight [C][up8(N)];
//   partial: pk_bn_bwd_blocks(rows) x 2 x C floats;  sums: 2 x C floats.
extern "C" int pk_bn_out1x1_bwd(const void* g, const void* raw, const uint8_t* relu_mask, const void* w_dgrad, const float* save_mean,
                                const float* save_rstd, const float* gamma, float* partial, float* sums, float* dgamma, float* dbeta, void* draw,
                                int64_t rows, int C, int N, void* stream) {
    PK_REQUIRE(g && raw && relu_mask && w_dgrad && save_mean && save_rstd && gamma && partial && sums && dgamma && dbeta && draw,
               "pk_bn_out1x1_bwd: null pointer");
    BO_CHECK_SHAPE("pk_bn_out1x1_bwd");
    PK_REQUIRE(bo_aligned(g, raw, w_dgrad, draw), "pk_bn_out1x1_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    BnOutArgs a{};
    a.raw = (const uint4*)raw;
    a.w = (const uint16_t*)w_dgrad;
    a.g = (const uint16_t*)g;
    a.mask_in = relu_mask;
    a.v0 = save_mean;
    a.v1 = save_rstd;
    a.part = partial;
    a.rows = rows;
    a.N = N;
    a.N8 = (N + 7) / 8 * 8;
    a.nb = pk_bn_bwd_blocks(rows);
    a.rpb = (int)((rows + a.nb - 1) / a.nb);
    if (int rc = bo_bwd_any<1>(a, C, st, "pk_bn_out1x1_bwd (reduce)")) return rc;
    const int small = rows <= BO_SMALL_ROWS;
    if (small) hipLaunchKernelGGL(k_bn_out1x1_sum_small, dim3((unsigned)((C + 31) / 32)), dim3(256), 0, st, partial, a.nb, C, sums, dbeta, dgamma);
    else sum_partials_launch(partial, a.nb, 2 * C, 2 * C, sums, 1.f, 0, dbeta, dgamma, C, st);
    a.gamma = gamma;
    a.sums = sums;
    a.inv_count = 1.f / (float)rows;
    a.small = small;
    a.draw = (uint4*)draw;
    return bo_bwd_any<2>(a, C, st, "pk_bn_out1x1_bwd (apply)");
}
