// 1x1 convolution 64 -> 256 channels with BatchNorm around it, the pre-normalisation tensor never stored: layer1's conv3 + bn3 and its
// downsample branch (models/_blocks.py), 196 608 rows at 256x192, B = 64.  `raw` = bf16(x W^T) is 100.7 MB there and existed only so that
// BatchNorm could read it again (once forward, twice backward); its producer input is 25.2 MB and the contraction is 64 deep, so every
// pass below recomputes the tile it needs: 2 MFMAs per 16 x 16 block.
//
// One body, four epilogues (MODE):
//   0  statistics only: per 128-row tile the column sums / sums of squares of the fp32 accumulators, [tiles][2][256], what pk_bn_finalize reads
//   1  forward apply:   y = act(bf16(conv) * scale + shift (+ residual)), ReLU bit mask                       (k_bn_act on a stored raw)
//   2  backward reduce: partial sums of g and g * xhat, g = dy masked by the ReLU bits, in k_bn_bwd_reduce's split and order (one wave
//                       per partial row): the partial rows, and so sums, dgamma, dbeta and draw, are pk_bn_bwd's bit for bit
//   3  backward apply:  draw = gamma rstd (g - sum_g / M - xhat sum_gx / M), optional dresidual = g           (k_bn_bwd_apply)
//
// Body: a ROW PANEL of 128 pixels x all 256 output channels per tile, persistent workgroups (256 threads = 4 waves, 32 rows per wave)
// walking tiles bid, bid + grid, ...  The packed weight [256][64] bf16 (32 KB) is staged in LDS once per workgroup (16-byte chunks
// XOR-swizzled by (row >> 1) & 7, the conflict-free pattern of k_igemm2's 128-byte rows).  The x fragments of a wave's 32 rows come
// straight from global memory (a row is 128 contiguous bytes, 16 per lane) and are held for the whole tile; every weight fragment read from
// LDS feeds both 16-row blocks.  Same instruction (v_mfma_f32_16x16x32_bf16, weights as the A operand), same k -> lane assignment and same
// K-chunk order (channels 0..31, then 32..63) as k_igemm2: the accumulators, and so the bf16-rounded raw values, are bit for bit what
// pk_conv2d_nhwc stores.  The 256 channels are walked in four groups of 64; a group's accumulators go through a wave-private fp32 LDS
// tile so that every global access to a 256-channel tensor is a 16-byte-per-lane access covering whole 128-byte row segments.  The
// streamed operands (dy, residual, mask bytes) of the NEXT channel group -- across tiles too -- and the x fragments of the next tile are
// requested before the current group is computed.
//
// Fixed orders everywhere (no atomics): two launches give identical bytes, and a training step computes what it computed with the
// stored raw.  No grid-wide barrier, no spin-wait.
#include <stdlib.h>

#include "pk_rowops.h"

#define CB_ROWS 128
#define CB_CIN 64
#define CB_COUT 256
#define CB_EP 68                                        // fp32 pitch of the staging tile (64 + 4: conflict-free b128 rows, as in k_igemm2)
#define CB_W_BYTES (CB_COUT * CB_CIN * 2)               // 32 768
#define CB_STAGE_BYTES (4 * 32 * CB_EP * 4)             // 34 816: 32 rows x 64 channels per wave (MODE 0: [4][256][2] statistics scratch)
#define CB_VEC_BYTES (5 * CB_COUT * 4)                  // per-channel vectors of the epilogue
#define CB_LDS (CB_W_BYTES + CB_STAGE_BYTES + CB_VEC_BYTES)
#define CB_GRID 512                                     // two workgroups per CU (2 x 72 704 bytes of LDS)
#define CB_MIN_ROWS 32768                               // from here pk_bn_train_fwd / pk_bn_bwd take their large-tensor form (pk_bn.hip)

struct Conv1x1Args {
    const uint16_t* x;          // [rows][64] bf16
    const uint16_t* w;          // [256][1][64] bf16, the packed forward weight
    const uint4* in;            // MODE 1: residual or null; MODE 2, 3: dy
    const uint8_t* mask_in;     // MODE 2, 3: ReLU bits (relu != 0)
    const float* v0;            // MODE 1: scale;  MODE 2, 3: mean
    const float* v1;            // MODE 1: shift;  MODE 2, 3: rstd
    const float* gamma;         // MODE 3
    const float* sums;          // MODE 3: [2][256]
    uint4* out;                 // MODE 1: y;  MODE 3: draw
    uint4* out2;                // MODE 3: dresidual or null
    uint8_t* mask_out;          // MODE 1: ReLU bits or null
    float* part;                // MODE 0: [tiles][2][256];  MODE 2: [nb][2][256]
    float inv_count;            // MODE 3
    int64_t rows;
    int relu;
    int nb, rpb;                // MODE 2: partial rows and rows per partial row, the split of k_bn_bwd_reduce
};

template <int MODE>
__global__ void __launch_bounds__(256, 2) k_conv1x1_bn(Conv1x1Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cb_smem[];
    uint16_t* sW = reinterpret_cast<uint16_t*>(cb_smem);
    float* sStage = reinterpret_cast<float*>(cb_smem + CB_W_BYTES);
    float* sVec = reinterpret_cast<float*>(cb_smem + CB_W_BYTES + CB_STAGE_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fkc = lane >> 4;
    const int64_t rows = p.rows;
    const int ntiles = (int)((rows + CB_ROWS - 1) / CB_ROWS);
    const int lr = lane >> 3, lc = (lane & 7) * 8;        // epilogue: row of a pass of 8, first of the lane's 8 channels inside the group
    float* stage = sStage + wave * 32 * CB_EP;
    auto wave_sync = [] {                                  // the staging tile is wave-private (see k_igemm2's epilogue)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    // A wave works on 32 consecutive rows [base, base + 32) cut at `end`: its quarter of a 128-row tile (MODE 0, 1, 3), or the next 32 rows
    // of the partial row it is summing (MODE 2).
    auto load_x = [&](bf16x8 (&xf)[2][2], int64_t base, int64_t end) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t row = base + b * 16 + frow;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (row < end) v = *reinterpret_cast<const bf16x8*>(p.x + (size_t)row * CB_CIN + ks * 32 + fkc * 8);
                xf[ks][b] = v;
            }
        }
    };
    // streamed operands of (rows, channel group): this lane's 16-byte chunk of rows lr, lr + 8, lr + 16, lr + 24 of the wave's 32
    auto load_in = [&](uint4 (&iv)[4], uint32_t (&mv)[4], int64_t base, int64_t end, int cg) {
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int64_t row = base + ps * 8 + lr;
            const size_t idx = (size_t)row * (CB_COUT / 8) + cg * 8 + (lane & 7);
            iv[ps] = make_uint4(0u, 0u, 0u, 0u);
            mv[ps] = 0xffu;
            if (row < end) {
                if (MODE >= 2 || (MODE == 1 && p.in)) iv[ps] = p.in[idx];
                if (MODE >= 2 && p.relu) mv[ps] = p.mask_in[idx];
            }
        }
    };

    // MODE 2 reproduces k_bn_bwd_reduce's sums bit for bit: one WAVE per partial row u (rows [u rpb, (u + 1) rpb), 32 at a time in
    // ascending order), lane row lr = that kernel's row lane (rows u rpb + lr + 8 i, added in ascending order), then the eight row lanes
    // in order -- so that the summed partial rows, and with them draw, are what pk_bn_bwd computes from a stored raw.
    auto position = [&](int t, int u, int k, int64_t& base, int64_t& end) {
        if (MODE == 2) {
            base = end = 0;                                // past the last partial row: nothing is read
            if (u < p.nb) {
                base = (int64_t)u * p.rpb + 32 * k;
                end = min(rows, (int64_t)(u + 1) * p.rpb);
            }
        } else {
            base = (int64_t)t * CB_ROWS + wave * 32;       // at or beyond ntiles: every row fails `row < end`
            end = rows;
        }
    };
    float s1[4][8], s2[4][8];                              // MODE 2: this lane's sums over the rows of one partial row
    if (MODE == 2) {
#pragma unroll
        for (int cg = 0; cg < 4; ++cg)
#pragma unroll
            for (int j = 0; j < 8; ++j) s1[cg][j] = s2[cg][j] = 0.f;
    }

    bf16x8 xf[2][2], xn[2][2];
    uint4 iv[2][4];
    uint32_t mv[2][4];
    int tile = (int)blockIdx.x, sbuf = 0;
    int unit = (int)blockIdx.x * 4 + wave, chunk = 0;
    int64_t base, end;
    position(tile, unit, chunk, base, end);
    load_x(xf, base, end);
    if (MODE >= 1) load_in(iv[0], mv[0], base, end, 0);
    // (the first tile's operands are requested before the weight is staged: their HBM latency runs under the staging)
    // ---- once per workgroup: the weight and the per-channel vectors
    for (int i = tid; i < CB_COUT * (CB_CIN / 8); i += 256) {
        const int row = i >> 3, ch = i & 7;
        *reinterpret_cast<u32x4*>(&sW[row * CB_CIN + ((ch ^ ((row >> 1) & 7)) * 8)]) = reinterpret_cast<const u32x4*>(p.w)[i];
    }
    if (MODE >= 1) {
        sVec[tid] = p.v0[tid];
        sVec[CB_COUT + tid] = p.v1[tid];
    }
    if (MODE == 3) {
        sVec[2 * CB_COUT + tid] = p.gamma[tid];
        sVec[3 * CB_COUT + tid] = p.sums[tid];
        sVec[4 * CB_COUT + tid] = p.sums[CB_COUT + tid];
    }
    __syncthreads();
    while (MODE == 2 ? unit < p.nb : tile < ntiles) {      // (MODE 2: per wave, no workgroup barrier inside; else uniform over the workgroup)
        const bool unit_done = MODE == 2 && base + 32 >= end;
        const int tile_next = tile + (int)gridDim.x;
        const int unit_next = unit_done ? unit + (int)gridDim.x * 4 : unit, chunk_next = unit_done ? 0 : chunk + 1;
        int64_t nbase, nend;
        position(tile_next, unit_next, chunk_next, nbase, nend);
        load_x(xn, nbase, nend);
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) {
            if (MODE >= 1) {
                if (cg < 3) load_in(iv[(cg + 1) & 1], mv[(cg + 1) & 1], base, end, cg + 1);
                else load_in(iv[0], mv[0], nbase, nend, 0);
            }
            f32x4 acc[4][2];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 wf[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int n = cg * 64 + a * 16 + frow;
                    wf[a] = *reinterpret_cast<const bf16x8*>(&sW[n * CB_CIN + (((fkc + 4 * ks) ^ ((n >> 1) & 7)) * 8)]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a], xf[ks][b], acc[a][b], 0, 0, 0);
            }
            if (MODE == 0) {
                // the statistics epilogue of k_igemm2<128, 64, 4, 1, 32, .>: per wave the two 16-row blocks, then the 16 pixel lanes,
                // then (below) the four waves in order
                float* sStat = sStage + sbuf * (4 * CB_COUT * 2);      // [wave][256][2], two buffers: one barrier per tile
#pragma unroll
                for (int a = 0; a < 4; ++a) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float s = 0.f, q = 0.f;
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const float v = acc[a][b][r];
                            s += v;
                            q += v * v;
                        }
                        s = row16_sum(s);
                        q = row16_sum(q);
                        if (frow == 0) {
                            const int nl = cg * 64 + a * 16 + fkc * 4 + r;
                            sStat[(wave * CB_COUT + nl) * 2] = s;
                            sStat[(wave * CB_COUT + nl) * 2 + 1] = q;
                        }
                    }
                }
                continue;
            }
            // ---- accumulators -> wave-private fp32 tile -> 8-channel row segments
            wave_sync();                                   // the previous group has been read out
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int a = 0; a < 4; ++a) *reinterpret_cast<f32x4*>(&stage[(b * 16 + frow) * CB_EP + a * 16 + fkc * 4]) = acc[a][b];
            wave_sync();
            const int c0 = cg * 64 + lc;
            float va[8], vb[8], vc[8], vd[8], ve[8];       // the lane's 8 channels of the per-channel vectors
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                va[j] = sVec[c0 + j];
                vb[j] = sVec[CB_COUT + c0 + j];
                if (MODE == 3) {
                    vc[j] = sVec[2 * CB_COUT + c0 + j];
                    vd[j] = sVec[3 * CB_COUT + c0 + j];
                    ve[j] = sVec[4 * CB_COUT + c0 + j];
                }
            }
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int ml = ps * 8 + lr;
                const int64_t row = base + ml;
                if (row >= end) continue;
                const size_t idx = (size_t)row * (CB_COUT / 8) + cg * 8 + (lane & 7);
                const f32x4 lo = *reinterpret_cast<const f32x4*>(&stage[ml * CB_EP + lc]);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(&stage[ml * CB_EP + lc + 4]);
                const float accv[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                float xr[8];
                unpack8(pack8(accv), xr);                  // raw as the conv stores it and BatchNorm reads it back
                const uint4 in = iv[cg & 1][ps];
                if (MODE == 1) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = xr[j] * va[j] + vb[j];
                    if (p.in) {                            // (workgroup-uniform branches around whole 8-channel loops: packed fp32 math inside)
                        float r[8];
                        unpack8(in, r);
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] += r[j];
                    }
                    if (p.relu) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
                    }
                    const uint4 o = pack8(v);
                    p.out[idx] = o;
                    if (p.mask_out) p.mask_out[idx] = (uint8_t)pos_mask8(o);
                } else {
                    float g[8];
                    unpack8(in, g);
                    const uint32_t mb = mv[cg & 1][ps];
                    if (MODE == 2) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float gg = ((mb >> j) & 1u) ? g[j] : 0.f;
                            s1[cg][j] += gg;
                            s2[cg][j] += gg * (xr[j] - va[j]) * vb[j];
                        }
                    } else {
                        float o[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float gg = ((mb >> j) & 1u) ? g[j] : 0.f;
                            g[j] = gg;
                            const float xh = (xr[j] - va[j]) * vb[j];
                            o[j] = vc[j] * vb[j] * (gg - vd[j] * p.inv_count - xh * ve[j] * p.inv_count);
                        }
                        p.out[idx] = pack8(o);
                        if (p.out2) p.out2[idx] = pack8(g);
                    }
                }
            }
        }
        if (MODE == 0) {
            __syncthreads();                               // (a buffer is rewritten two tiles later: behind the next tile's barrier)
            const float* sStat = sStage + sbuf * (4 * CB_COUT * 2);
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                s += sStat[(w * CB_COUT + tid) * 2];
                q += sStat[(w * CB_COUT + tid) * 2 + 1];
            }
            float* dst = p.part + (size_t)tile * 2 * CB_COUT;
            dst[tid] = s;
            dst[CB_COUT + tid] = q;
            sbuf ^= 1;
        }
        if (MODE == 2 && unit_done) {
            // the eight row lanes of every channel, in order, through the wave's staging tile ([lr][2][64] floats per channel group)
            float* dst = p.part + (size_t)unit * 2 * CB_COUT;
#pragma unroll
            for (int cg = 0; cg < 4; ++cg) {
                wave_sync();
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    stage[(lr * 2) * 64 + lc + j] = s1[cg][j];
                    stage[(lr * 2 + 1) * 64 + lc + j] = s2[cg][j];
                    s1[cg][j] = s2[cg][j] = 0.f;
                }
                wave_sync();
                float a = 0.f, b = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    a += stage[(k * 2) * 64 + lane];
                    b += stage[(k * 2 + 1) * 64 + lane];
                }
                dst[cg * 64 + lane] = a;
                dst[CB_COUT + cg * 64 + lane] = b;
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int b = 0; b < 2; ++b) xf[ks][b] = xn[ks][b];
        tile = tile_next;
        unit = unit_next;
        chunk = chunk_next;
        base = nbase;
        end = nend;
    }
}

// ================================================================================================ routing and entries
// Three per-call switches, after the PK_CONV8P* precedent: PK_CONV1X1_BN=0 turns the route off, PK_CONV1X1_BN_MIN_ROWS lowers the row
// threshold (the tests reach small and ragged shapes with it), PK_CONV1X1_BN_MAX_GRID caps the workgroups of a launch (a small problem
// then makes a workgroup walk several tiles).
static inline int cb_grid(int64_t rows) {
    const char* cap = getenv("PK_CONV1X1_BN_MAX_GRID");
    int64_t g = (rows + CB_ROWS - 1) / CB_ROWS;
    int64_t lim = CB_GRID;
    if (cap && atoi(cap) >= 1 && atoi(cap) < CB_GRID) lim = atoi(cap);
    if (g > lim) g = lim;
    return (int)(g < 1 ? 1 : g);
}
extern "C" int pk_conv1x1_bn_supported(int64_t rows, int Cin, int Cout) {
    const char *on = getenv("PK_CONV1X1_BN"), *mr = getenv("PK_CONV1X1_BN_MIN_ROWS");
    if (on && on[0] == '0') return 0;
    int64_t min_rows = CB_MIN_ROWS;
    if (mr && atoll(mr) >= 1) min_rows = atoll(mr);
    return (Cin == CB_CIN && Cout == CB_COUT && rows >= min_rows && rows < (1 << 30)) ? 1 : 0;
}
extern "C" int pk_conv1x1_stats_rows(int64_t rows) { return rows > 0 && rows < (1 << 30) ? (int)((rows + CB_ROWS - 1) / CB_ROWS) : 0; }
// partial rows of the backward reduce: pk_bn_bwd's own split (pk_bn_bwd_blocks), reproduced row for row
extern "C" int pk_conv1x1_bn_bwd_rows(int64_t rows) { return rows > 0 && rows < (1 << 30) ? pk_bn_bwd_blocks(rows) : 0; }

static inline bool cb_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}
#define CB_CHECK_SHAPE(who)                                                                                                       \
    PK_REQUIRE(rows > 0 && rows < (1 << 30), who ": bad row count");                                                             \
    PK_SUPPORTED(Cin == CB_CIN && Cout == CB_COUT, who ": built for Cin = 64, Cout = 256 (got %d -> %d)", Cin, Cout)

template <int MODE>
static int cb_launch(const Conv1x1Args& a, hipStream_t st, const char* who) {
    // more than 64 KB of LDS: asked for once per kernel (during the eager warm-up steps, not inside a graph capture)
    static bool attr_set = false;
    const hipError_t e = attr_set ? hipSuccess : hipFuncSetAttribute((const void*)k_conv1x1_bn<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, CB_LDS);
    if (e != hipSuccess) return pk_set_error("%s: cannot reserve %d bytes of LDS: %s", who, CB_LDS, hipGetErrorString(e)), (int)e;
    attr_set = true;
    // MODE 2: one wave per partial row, four to a workgroup; else one workgroup per 128-row tile; both up to the cap
    const int grid = MODE == 2 ? cb_grid((int64_t)a.nb * 32) : cb_grid(a.rows);
    hipLaunchKernelGGL(k_conv1x1_bn<MODE>, dim3((unsigned)grid), dim3(256), CB_LDS, st, a);
    return pk_launch_status(who);
}

extern "C" int pk_conv1x1_stats(const void* x, const void* w, float* stats_partial, int64_t rows, int Cin, int Cout, void* stream) {
    PK_REQUIRE(x && w && stats_partial, "pk_conv1x1_stats: null pointer");
    CB_CHECK_SHAPE("pk_conv1x1_stats");
    PK_REQUIRE(cb_aligned(x, w), "pk_conv1x1_stats: x and w must be 16-byte aligned");
    Conv1x1Args a{};
    a.x = (const uint16_t*)x;
    a.w = (const uint16_t*)w;
    a.part = stats_partial;
    a.rows = rows;
    return cb_launch<0>(a, (hipStream_t)stream, "pk_conv1x1_stats");
}

extern "C" int pk_conv1x1_bn_act(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y, int relu,
                                 uint8_t* relu_mask, int64_t rows, int Cin, int Cout, void* stream) {
    PK_REQUIRE(x && w && scale && shift && y, "pk_conv1x1_bn_act: null pointer");
    CB_CHECK_SHAPE("pk_conv1x1_bn_act");
    PK_REQUIRE(cb_aligned(x, w, residual, y), "pk_conv1x1_bn_act: tensors must be 16-byte aligned");
    Conv1x1Args a{};
    a.x = (const uint16_t*)x;
    a.w = (const uint16_t*)w;
    a.v0 = scale;
    a.v1 = shift;
    a.in = (const uint4*)residual;
    a.out = (uint4*)y;
    a.mask_out = relu_mask;
    a.relu = relu ? 1 : 0;
    a.rows = rows;
    return cb_launch<1>(a, (hipStream_t)stream, "pk_conv1x1_bn_act");
}

extern "C" int pk_conv1x1_bn_bwd_reduce(const void* dy, const void* x, const void* w, const float* save_mean, const float* save_rstd,
                                        float* partial, int64_t rows, int Cin, int Cout, int relu, const uint8_t* relu_mask, void* stream) {
    PK_REQUIRE(dy && x && w && save_mean && save_rstd && partial, "pk_conv1x1_bn_bwd_reduce: null pointer");
    PK_REQUIRE(!relu || relu_mask, "pk_conv1x1_bn_bwd_reduce: relu needs the bit mask of the forward");
    CB_CHECK_SHAPE("pk_conv1x1_bn_bwd_reduce");
    PK_REQUIRE(cb_aligned(dy, x, w), "pk_conv1x1_bn_bwd_reduce: tensors must be 16-byte aligned");
    Conv1x1Args a{};
    a.x = (const uint16_t*)x;
    a.w = (const uint16_t*)w;
    a.in = (const uint4*)dy;
    a.mask_in = relu_mask;
    a.v0 = save_mean;
    a.v1 = save_rstd;
    a.part = partial;
    a.relu = relu ? 1 : 0;
    a.rows = rows;
    a.nb = pk_bn_bwd_blocks(rows);
    a.rpb = (int)((rows + a.nb - 1) / a.nb);
    return cb_launch<2>(a, (hipStream_t)stream, "pk_conv1x1_bn_bwd_reduce");
}

extern "C" int pk_conv1x1_bn_bwd_apply(const void* dy, const void* x, const void* w, const float* save_mean, const float* save_rstd,
                                       const float* gamma, const float* sums, float inv_count, void* draw, void* dresidual, int64_t rows, int Cin,
                                       int Cout, int relu, const uint8_t* relu_mask, void* stream) {
    PK_REQUIRE(dy && x && w && save_mean && save_rstd && gamma && sums && draw, "pk_conv1x1_bn_bwd_apply: null pointer");
    PK_REQUIRE(!relu || relu_mask, "pk_conv1x1_bn_bwd_apply: relu needs the bit mask of the forward");
    CB_CHECK_SHAPE("pk_conv1x1_bn_bwd_apply");
    PK_REQUIRE(cb_aligned(dy, x, w, draw) && cb_aligned(dresidual), "pk_conv1x1_bn_bwd_apply: tensors must be 16-byte aligned");
    Conv1x1Args a{};
    a.x = (const uint16_t*)x;
    a.w = (const uint16_t*)w;
    a.in = (const uint4*)dy;
    a.mask_in = relu_mask;
    a.v0 = save_mean;
    a.v1 = save_rstd;
    a.gamma = gamma;
    a.sums = sums;
    a.inv_count = inv_count;
    a.out = (uint4*)draw;
    a.out2 = (uint4*)dresidual;
    a.relu = relu ? 1 : 0;
    a.rows = rows;
    return cb_launch<3>(a, (hipStream_t)stream, "pk_conv1x1_bn_bwd_apply");
}

// pk_bn_bwd with (x, w) in place of raw: reduce, the fixed-order sum of the partial rows (sums = [sum g | sum g xhat], the same values to
// dbeta / dgamma), apply.  partial: pk_conv1x1_bn_bwd_rows(rows) x 2 x Cout floats; sums: 2 x Cout floats.
extern "C" int pk_conv1x1_bn_bwd(const void* dy, const void* x, const void* w, const float* save_mean, const float* save_rstd, const float* gamma,
                                 float* partial, float* sums, float* dgamma, float* dbeta, void* draw, void* dresidual, int64_t rows, int Cin,
                                 int Cout, int relu, const uint8_t* relu_mask, void* stream) {
    PK_REQUIRE(partial && sums && dgamma && dbeta && gamma && draw, "pk_conv1x1_bn_bwd: null pointer");
    if (int rc = pk_conv1x1_bn_bwd_reduce(dy, x, w, save_mean, save_rstd, partial, rows, Cin, Cout, relu, relu_mask, stream)) return rc;
    sum_partials_launch(partial, pk_bn_bwd_blocks(rows), 2 * CB_COUT, 2 * CB_COUT, sums, 1.f, 0, dbeta, dgamma, CB_COUT, (hipStream_t)stream);
    return pk_conv1x1_bn_bwd_apply(dy, x, w, save_mean, save_rstd, gamma, sums, 1.f / (float)rows, draw, dresidual, rows, Cin, Cout, relu, relu_mask,
                                   stream);
}
