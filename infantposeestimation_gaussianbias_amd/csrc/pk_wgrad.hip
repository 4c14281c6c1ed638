// Weight gradients on MFMA (bf16 in, fp32 accumulate) of every convolution and linear layer that pk_igemm.hip runs forward.
//
// This unit holds k_wgrad2 (register-staged), k_wgrad3 (LDS-DMA ring, the wide 3x3 convs of the head), the streaming kernels k_wgrad4 /
// k_wgrad4g (grouped) / k_wgrad4w (window-gathered, scaled rows) / k_wgrad4_3x3, the slab reductions k_wgrad_reduce and k_reduce_many,
// the routing functions that pick among them (wgrad_route, wgrad_group_route) and the entry points pk_wgrad_bf16, pk_wgrad_slices,
// pk_wgrad_group, pk_wgrad_group_slices and pk_reduce_many.
#include "pk_common.h"

// ================================================================================================ weight gradient
// dW[n][t][c] = sum_m G(m, n) * A(m, t, c).  The contraction runs over pixels/tokens m, i.e. along the ROWS of both
// operands as they sit in HBM, so each MFMA fragment needs 8 consecutive m of one column.  Tiles are staged row-major
// ([m][n] and [m][c], 16-byte global loads -> 16-byte LDS stores) and the fragments are read with the gfx950 hardware
// transpose read `ds_read_b64_tr_b16` (4 rows x 16 columns per 16-lane group, delivered column-major): two reads per
// fragment, no scalar LDS traffic.  Row pitch = width + 16 elements keeps those reads bank-conflict free.
// One workgroup owns a TN(n) x TC(c) tile of one filter tap and one slice of M (split-M over gridDim.z); slices are
// written as fp32 slabs and summed in fixed order by k_wgrad_reduce (deterministic, no float atomics).
struct WgradArgs {
    const uint16_t* x;   // activations (layer input) bf16
    const uint16_t* g;   // output gradient bf16 [rows][N]
    float* part;         // [S][N][T][Cin] fp32
    const int32_t* a_rowmap;  // source row of x for GEMM row m (linear), -1 = zero row
    const int32_t* g_rowmap;  // source row of g for GEMM row m, -1 = zero row
    const float* g_scale;     // optional per-sample multiplier of g rows (DropPath), indexed by g_row / g_rows_per_sample
    int g_rows_per_sample;
    float* bias_part;         // optional [S][N] fp32: column sums of the (scaled, gathered) G rows = bias gradient slabs
    int M, N, Cin, T, Hs, Ws, Ho, Wo, stride, pad, m_per_slice, ctiles;
    int ntiles3, nslices3;    // k_wgrad3: output tiles per tap, number of M-slices
};

#define WG_MK 32
__device__ __forceinline__ bf16x8 tr_frag(const uint16_t* tile, int pitch, int col0, int lane) {
    // fragment for MFMA lane (col = col0 + lane&15, k-group g = lane>>4): elements k = 8g .. 8g+7 of that column
    const int g = lane >> 4, i = lane & 15, q = i >> 2, pq = i & 3;
    const uint16_t* a0 = tile + (8 * g + q) * pitch + col0 + 4 * pq;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 4 * pitch));
    return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int TN, int TC, int MK>   // output tile: TN rows (n) x TC columns (c), 4 waves as 2 x 2; MK pixel rows staged per step
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TN == 128 && MK == 32 ? 4 : 1))) k_wgrad2(WgradArgs p) {
    constexpr int PN = TN + 16, PC = TC + 16;            // LDS row pitches (elements)
    constexpr int GCH = TN / 8, XCH = TC / 8;            // 16-byte chunks per staged row
    constexpr int G_PT = MK * GCH / 256, X_PT = MK * XCH / 256;   // chunks per thread per step (1 or 2)
    constexpr int NI = TN / 2 / 16, CI = TC / 2 / 16;    // accumulator tiles per wave
    __shared__ __attribute__((aligned(16))) uint16_t sG[2][MK * PN];
    __shared__ __attribute__((aligned(16))) uint16_t sX[2][MK * PC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 3x3: 1-D grid, the nine taps (and the output tiles) of one M-slice on ONE XCD (slice = xcd + 8 * group): they read the same
    // rows of G and overlapping rows of X at about the same time, so eight of the nine reads are L2 hits.
    int bx = blockIdx.x, t = blockIdx.y, bz = blockIdx.z;
    if (p.nslices3 > 0) {
        const int xcd = blockIdx.x & 7, k_in = blockIdx.x >> 3, per_slice = 9 * p.ntiles3;
        bz = xcd + 8 * (k_in / per_slice);
        if (bz >= p.nslices3) return;            // padding workgroups of the last group (whole workgroup, before any barrier)
        const int rem = k_in % per_slice;
        t = rem % 9;
        bx = rem / 9;
    }
    const int ntile = bx / p.ctiles, ctile = bx - ntile * p.ctiles;
    const int n0 = ntile * TN, c0 = ctile * TC;
    const int kw_n = (p.T == 9) ? 3 : 1, kh = t / kw_n, kw = t - kh * kw_n;
    const int m_begin = bz * p.m_per_slice;
    const int m_end = min(p.M, m_begin + p.m_per_slice);
    const bool linear = (p.Ho == 0);
    const int hw = p.Ho * p.Wo;
    const auto rx = MAKE_RSRC(p.x);
    const auto rg = MAKE_RSRC(p.g);

    // fixed (row-in-step, chunk) assignment
    int g_row[G_PT], g_col[G_PT], x_row[X_PT], x_col[X_PT];
#pragma unroll
    for (int i = 0; i < G_PT; ++i) { const int q = tid + 256 * i; g_row[i] = q / GCH; g_col[i] = (q % GCH) * 8; }
#pragma unroll
    for (int i = 0; i < X_PT; ++i) { const int q = tid + 256 * i; x_row[i] = q / XCH; x_col[i] = (q % XCH) * 8; }

    // The DropPath row scale is applied when the staged registers are written to LDS, not when they are loaded: scaling at
    // load time consumed the load result immediately and serialised every step of the proj / fc2 weight gradients on a
    // global-memory round trip.  (Tried and dropped: a second register set with loads two steps ahead -- the duplicated loop
    // body pushed the 128 x 128 tile into scratch, 523 -> 1 816 us, and bought nothing on the 64 x 64 tile.)
    u32x4 rgv[G_PT], rxv[X_PT];
    float rsc[G_PT];
    auto load = [&](int ms) {
#pragma unroll
        for (int i = 0; i < G_PT; ++i) {
            const int m = ms + g_row[i], n = n0 + g_col[i];
            unsigned off = OOB_OFF;
            float sc = 1.f;
            if (m < m_end && n < p.N) {
                const int gr = p.g_rowmap ? p.g_rowmap[m] : m;
                if (gr >= 0) {
                    off = (unsigned)((gr * p.N + n) * 2);
                    if (p.g_scale) sc = p.g_scale[gr / p.g_rows_per_sample];
                }
            }
            rgv[i] = __builtin_amdgcn_raw_buffer_load_b128(rg, off, 0, 0);
            rsc[i] = sc;
        }
#pragma unroll
        for (int i = 0; i < X_PT; ++i) {
            const int m = ms + x_row[i], c = c0 + x_col[i];
            unsigned off = OOB_OFF;
            if (m < m_end && c < p.Cin) {
                if (linear) {
                    const int xr = p.a_rowmap ? p.a_rowmap[m] : m;
                    if (xr >= 0) off = (unsigned)((xr * p.Cin + c) * 2);
                } else {
                    const int b = m / hw, r = m - b * hw, oy = r / p.Wo, ox = r - oy * p.Wo;
                    const int iy = oy * p.stride - p.pad + kh, ix = ox * p.stride - p.pad + kw;
                    if (iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws) off = (unsigned)((((b * p.Hs + iy) * p.Ws + ix) * p.Cin + c) * 2);
                }
            }
            rxv[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < G_PT; ++i) {
            u32x4 v = rgv[i];
            if (p.g_scale) {
                const float sc = rsc[i];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = pack_bf16x2(__uint_as_float(v[j] << 16) * sc, __uint_as_float(v[j] & 0xffff0000u) * sc);
            }
            *reinterpret_cast<u32x4*>(&sG[buf][g_row[i] * PN + g_col[i]]) = v;
        }
#pragma unroll
        for (int i = 0; i < X_PT; ++i) *reinterpret_cast<u32x4*>(&sX[buf][x_row[i] * PC + x_col[i]]) = rxv[i];
    };
    f32x4 acc[NI][CI];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < CI; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wn = wave >> 1, wc = wave & 1;
    const int nsteps = (m_end - m_begin + MK - 1) / MK;
    const bool do_bias = p.bias_part && ctile == 0 && t == 0;      // one workgroup column per n-tile owns the bias slab
    float bsum = 0.f;
    if (nsteps > 0) {
        load(m_begin);
        store(0);
    }
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) load(m_begin + (s + 1) * MK);
        if (do_bias && tid < TN) {          // column tid of the staged G tile: 32 rows, fixed order
#pragma unroll 8
            for (int r = 0; r < MK; ++r) bsum += bf16_to_f32(sG[buf][r * PN + tid]);
        }
#pragma unroll
        for (int ks = 0; ks < MK / 32; ++ks) {
            bf16x8 gf[NI], xf[CI];
#pragma unroll
            for (int a = 0; a < NI; ++a) gf[a] = tr_frag(sG[buf] + 32 * ks * PN, PN, wn * (TN / 2) + a * 16, lane);
#pragma unroll
            for (int b = 0; b < CI; ++b) xf[b] = tr_frag(sX[buf] + 32 * ks * PC, PC, wc * (TC / 2) + b * 16, lane);
#pragma unroll
            for (int a = 0; a < NI; ++a)
#pragma unroll
                for (int b = 0; b < CI; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[a], xf[b], acc[a][b], 0, 0, 0);
        }
        if (s + 1 < nsteps) store(buf ^ 1);
        __syncthreads();
    }
    if (do_bias && tid < TN && n0 + tid < p.N) p.bias_part[(size_t)bz * p.N + n0 + tid] = bsum;
    float* dst = p.part + (size_t)bz * p.N * p.T * p.Cin;
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < CI; ++b) {
            const int c = c0 + wc * (TC / 2) + b * 16 + (lane & 15);
            const int n = n0 + wn * (TN / 2) + a * 16 + (lane >> 4) * 4;
            if (c < p.Cin) {
                if (n < p.N) dst[((size_t)n * p.T + t) * p.Cin + c] = acc[a][b][0];
                if (n + 1 < p.N) dst[((size_t)(n + 1) * p.T + t) * p.Cin + c] = acc[a][b][1];
                if (n + 2 < p.N) dst[((size_t)(n + 2) * p.T + t) * p.Cin + c] = acc[a][b][2];
                if (n + 3 < p.N) dst[((size_t)(n + 3) * p.T + t) * p.Cin + c] = acc[a][b][3];
            }
        }
}

// ------------------------------------------------------------------------------------------------ wide weight-gradient kernel
// The 3x3 convolutions of the fusion head (256 -> 256 channels at 64x48, M = 196 608 pixels: 232 GFLOP each, five per step) ran
// at 19 % of the MFMA peak on the 128 x 128 tile above: every (n-tile, c-tile, tap) workgroup streams its slice of G and X again
// (36 x 100 MB per launch), 16 KB per 64 MFMAs = the CU's 64 B/clk L1 port at full MFMA rate, and a one-step register
// prefetch does not cover an L2 round trip.  This kernel:
//   * 256 (n) x 256 (c) output tile per 512-thread workgroup (8 waves as 4 x 2, 64 x 128 per wave: 128 accumulator registers):
//     twice the MFMAs per staged byte, operand traffic 18 x 100 MB;
//   * operands go global -> LDS by LDS-DMA (`buffer_load ... lds`, no VGPR round trip) into a FOUR-stage ring, three 32-row
//     K-steps in flight ahead of the one being multiplied, one raw s_barrier per step with a counted `s_waitcnt vmcnt`, so the
//     DMA stays in flight across the barrier;
//   * tiles are row-major [32 rows][256 columns] (512-byte rows, what one DMA wave-instruction writes linearly: two rows per
//     1 KiB piece) with the 16-byte chunks XOR-swizzled on the SOURCE side by swz(row) = 2 (row & 3) + 8 ((row >> 3) & 1): the
//     transpose reads `ds_read_b64_tr_b16` of a 32-lane half (rows r..r+3 and r+8..r+11, 32 columns) then touch 32 distinct
//     8-byte bank pairs (without it all rows alias: 8-way conflicts).
// One workgroup per CU (128 KB of LDS), 1-D grid of 9 taps x S slices ~ one round of workgroups with equal work.
// (Measured and dropped: software-pipelining the fragment reads of step s + 1 under the MFMAs of step s inside every wave -- behind the
// per-step barrier the eight waves read together and multiply together -- needs a second register set for G (and X): 128 accumulators
// + 64..80 fragment registers + addresses do not fit 256 VGPRs at two waves per SIMD; 110 spills, and scratch traffic shares vmcnt
// with the DMA ring.)
// LDS reads of tiles that are filled by LDS-DMA go through inline assembly.  The compiler cannot tell which LDS bytes an outstanding
// `buffer_load ... lds` will write, so before any ds_read it can see it inserts `s_waitcnt vmcnt(0)`: the tile requested a moment ago
// is awaited BEFORE the current one is multiplied: a four-deep ring is drained on every step (first version of k_wgrad3: 25 % of
// the MFMA peak, 372 us; 289 us with the reads below).  The kernels do their own accounting
// (counted vmcnt / barrier before a stage is read), read through ring_tr(), and close each group of reads with a fence that waits
// for the LDS data and, by naming the fragments as in/out operands, keeps the MFMAs behind it.
__device__ __forceinline__ s16x4 ring_tr(const uint16_t* a) {
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)a) : "memory");
    return v;
}
__device__ __forceinline__ void ring_fence(s16x4& a, s16x4& b, s16x4& c, s16x4& d, s16x4& e, s16x4& f, s16x4& g, s16x4& h) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h)::"memory");
}
__device__ __forceinline__ bf16x8 ring_join(const s16x4& lo, const s16x4& hi) {
    return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
#define W3_ROWS 32
#define W3_STAGES 5
__device__ __forceinline__ int w3_swz(int row) { return 2 * (row & 3) + 8 * ((row >> 3) & 1); }
__device__ __forceinline__ void w3_frag(const uint16_t* tile, int col0, int lane, s16x4& lo, s16x4& hi) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, pq = i & 3;
    const int row = 8 * g + q;
    const int pchunk = ((col0 >> 3) + (pq >> 1)) ^ (2 * q + 8 * (g & 1));          // w3_swz(row) == w3_swz(row + 4)
    const uint16_t* a0 = tile + row * 256 + pchunk * 8 + (pq & 1) * 4;
    lo = ring_tr(a0);
    hi = ring_tr(a0 + 4 * 256);
}
__global__ void __launch_bounds__(512, 2) k_wgrad3(WgradArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint16_t w3_smem[];            // [stage][G tile 32 x 256 | X tile 32 x 256]
    constexpr int TILE = W3_ROWS * 256;                                            // elements per operand tile (16 KB)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wc = wave & 1;
    // XCD-aware placement (1-D grid): workgroups are dealt to the 8 XCDs round-robin by linear id, each XCD has its own 4 MB L2.  The 9
    // taps (and the output tiles) of one M-slice read the same rows of G and X at about the same time, so they all go to ONE XCD
    // (slice z = xcd + 8 * group).
    const int xcd = blockIdx.x & 7, k_in = blockIdx.x >> 3, per_slice = 9 * p.ntiles3;
    const int zslice = xcd + 8 * (k_in / per_slice), rem = k_in % per_slice;
    if (zslice >= p.nslices3) return;            // padding workgroups of the last group (whole workgroup: no barrier was reached)
    const int t = rem % 9, tile3 = rem / 9;
    const int ntile = tile3 / p.ctiles, ctile = tile3 - ntile * p.ctiles;
    const int n0 = ntile * 256, c0 = ctile * 256;
    const int kh = t / 3, kw = t - kh * 3;
    const int m_begin = zslice * p.m_per_slice;
    const int m_end = min(p.M, m_begin + p.m_per_slice);
    const int nsteps = (max(m_end - m_begin, 0) + W3_ROWS - 1) / W3_ROWS;
    const int hw = p.Ho * p.Wo;
    const auto rx = MAKE_RSRC(p.x);
    const auto rg = MAKE_RSRC(p.g);
    // this wave's DMA pieces: tile rows (4 wave + 2 j, + 1), j = 0, 1; lane -> (row within the pair, physical chunk).  The pixel
    // coordinates of the lane's row are carried from step to step (+32 rows with carries): the first version recomputed them with two
    // integer divisions per piece and step, ~200 VALU instructions per wave and step -- more issue time than the step's 32 MFMAs.
    const int prow = lane >> 5, pchunk = lane & 31;
    int pm[2], pb[2], poy[2], pox[2], colg[2], colx[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = 4 * wave + 2 * j + prow;
        const int lch = pchunk ^ w3_swz(row);
        pm[j] = m_begin + row;
        pb[j] = pm[j] / hw;
        const int r = pm[j] - pb[j] * hw;
        poy[j] = r / p.Wo;
        pox[j] = r - poy[j] * p.Wo;
        colg[j] = n0 + lch * 8;
        colx[j] = c0 + lch * 8;
    }
    int issued = 0;
    auto issue_next = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)
        const int st = issued;
        issued = issued == W3_STAGES - 1 ? 0 : issued + 1;
        uint16_t* sg = w3_smem + st * 2 * TILE;
        uint16_t* sx = sg + TILE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool live = pm[j] < m_end;
            const int iy = poy[j] * p.stride - p.pad + kh, ix = pox[j] * p.stride - p.pad + kw;
            const bool in = live && iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws;
            const unsigned og = live ? (unsigned)((pm[j] * p.N + colg[j]) * 2) : OOB_OFF;
            const unsigned ox_ = in ? (unsigned)((((pb[j] * p.Hs + iy) * p.Ws + ix) * p.Cin + colx[j]) * 2) : OOB_OFF;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, (__attribute__((address_space(3))) void*)(sg + (4 * wave + 2 * j) * 256), 16, og, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(sx + (4 * wave + 2 * j) * 256), 16, ox_, 0, 0, 0);
            pm[j] += W3_ROWS;                       // next step: 32 rows further, with carries into (oy, b)
            pox[j] += W3_ROWS;
            while (pox[j] >= p.Wo) {
                pox[j] -= p.Wo;
                if (++poy[j] == p.Ho) {
                    poy[j] = 0;
                    ++pb[j];
                }
            }
        }
#endif
    };
    f32x4 acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // prologue: three steps in flight (steps beyond the slice issue out-of-range loads = zero tiles, so the counts stay uniform)
    issue_next();
    issue_next();
    issue_next();
    // ONE barrier per step, the two waves of every SIMD (wave groups 0-3 / 4-7) in opposite order between two barriers (k_conv8p has the
    // hazard analysis): group 0 [reads + DMA issue of step s; 32 MFMAs of step s], group 1 [32 MFMAs of step s-1 from the fragments it
    // read in the previous interval; reads + DMA issue of step s].  Step s+3 goes into the stage of step s-2, whose reads group 1 fenced
    // at the start of the previous interval: FIVE stages.  The counted wait (this wave's pieces of step s+1 landed, s+2 and s+3 may be
    // in flight) sits in front of the barrier that lets anyone read step s+1.  (Before: every wave read, then every wave multiplied,
    // behind one barrier per step -- the matrix pipe idled during each read phase: 300 us for the head conv.)
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int grp = __builtin_amdgcn_readfirstlane(wave >> 2);
    s16x4 gl[4], gh[4], xl[8], xh[8];
    auto multiply = [&]() {
        ring_fence(gl[0], gh[0], gl[1], gh[1], gl[2], gh[2], gl[3], gh[3]);
        ring_fence(xl[0], xh[0], xl[1], xh[1], xl[2], xh[2], xl[3], xh[3]);
        ring_fence(xl[4], xh[4], xl[5], xh[5], xl[6], xh[6], xl[7], xh[7]);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        bf16x8 gf[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) gf[a] = ring_join(gl[a], gh[a]);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bf16x8 xf = ring_join(xl[b], xh[b]);
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[a], xf, acc[a][b], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };
    int st_r = 0;
    for (int s = 0; s <= nsteps; ++s) {
        if (grp == 1 && s > 0) multiply();                          // group 1: step s-1
        if (s < nsteps) {
            const uint16_t* sg = w3_smem + st_r * 2 * TILE;
            const uint16_t* sx = sg + TILE;
#pragma unroll
            for (int a = 0; a < 4; ++a) w3_frag(sg, wn * 64 + a * 16, lane, gl[a], gh[a]);
#pragma unroll
            for (int b = 0; b < 8; ++b) w3_frag(sx, wc * 128 + b * 16, lane, xl[b], xh[b]);
            issue_next();                                           // step s+3 (zero tiles beyond the slice)
            __builtin_amdgcn_sched_barrier(0);
            if (grp == 0) multiply();                               // group 0: step s
        }
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        st_r = st_r == W3_STAGES - 1 ? 0 : st_r + 1;
        __builtin_amdgcn_s_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the run-ahead zero tiles must have landed before the LDS is released
    float* dst = p.part + (size_t)zslice * p.N * p.T * p.Cin;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int c = c0 + wc * 128 + b * 16 + (lane & 15);
            const int n = n0 + wn * 64 + a * 16 + (lane >> 4) * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[((size_t)(n + r) * p.T + t) * p.Cin + c] = acc[a][b][r];
        }
}

// ------------------------------------------------------------------------------------------------ streaming weight-gradient kernels
// Most weight gradients of the backbone are skinny GEMMs: M = 3 072 .. 219 520 rows against an N x Cin output of 32 .. 1 024 per
// side, i.e. a few flops per operand byte -- streaming work.  k_wgrad2 stages through registers one step ahead, so a workgroup
// covers a fraction of one memory round trip per step and the launcher needs >= 2 048 short slices to hide it; every slice writes
// a whole fp32 copy of its output tile (2.2 GB of slabs per step, read again by k_reduce_many).  k_wgrad4 keeps the k_wgrad3
// machinery (LDS-DMA ring with counted vmcnt across one raw barrier per step, source-side XOR swizzle, transpose reads) on
// 64/128-wide tiles with 256 threads and two workgroups per CU: 3 (ring of 4) or 7 (ring of 8) steps in flight per workgroup, so
// ~512 long slices fill the chip and the slab volume drops with the slice count.
//   k_wgrad4<TN, TC>: single tap (linear layers, 1x1 convolutions), bias gradient = one extra MFMA against a ones fragment.
//   k_wgrad4_3x3:     3x3 stride-1 convolutions, ALL NINE TAPS from one pass over G and X.  The K loop runs over PADDED pixel
//     coordinates p = (b, py, px) of the (Hs+2) x (Ws+2) zero-bordered image: dW[n][kh][kw][c] = sum_p Gpad[p][n] * Xpad[p + (kh-1)
//     (Ws+2) + (kw-1)][c], Gpad = 0 on the border, so every tap is the SAME 32 rows of G against a row-shifted window of one
//     circular X buffer (256 rows: 51 rows of halo either side + the rows in flight); border rows are fetched with the
//     out-of-range buffer offset (the DMA writes zeros).  64 x 64 output tile x 9 taps = 144 accumulator registers, waves split
//     the c range so each wave reads 4 G fragments + 9 X fragments for 36 MFMAs.
template <int W> __device__ __forceinline__ int w4_swz(int row) {            // in 16-byte chunks; uses row bits 0, 1, 3 only
    return W == 128 ? 2 * (row & 3) + 8 * ((row >> 3) & 1) : 2 * ((row >> 1) & 1) + 4 * ((row >> 3) & 1);
}
template <int W> __device__ __forceinline__ int w4_elem(int row, int col0, int pq) {
    return row * W + ((((col0 >> 3) + (pq >> 1)) ^ w4_swz<W>(row)) << 3) + (pq & 1) * 4;
}
template <int W> __device__ __forceinline__ void w4_frag(const uint16_t* tile, int col0, int lane, s16x4& lo, s16x4& hi) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, pq = i & 3;
    const uint16_t* a0 = tile + w4_elem<W>(8 * g + q, col0, pq);             // rows r and r + 4 share the swizzle (bit 2 is not used)
    lo = ring_tr(a0);
    hi = ring_tr(a0 + 4 * W);
}
__device__ __forceinline__ void ring_fence4(s16x4& a, s16x4& b, s16x4& c, s16x4& d) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
template <int N> __device__ __forceinline__ void w4_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
#define W4_LDS(ptr) ((__attribute__((address_space(3))) void*)(ptr))

// COLS = true ("column form", 3x3 convolutions the nine-tap kernel does not take: stride 2, or stride 1 on wide images): the X operand
// is the im2col matrix [M output pixels][9 * Cin], never materialised -- the lane that stages 16-byte chunk j of a row fetches
// tap j / (Cin / 8), channels 8 (j % (Cin / 8)) of that pixel's window (its own source address per DMA lane, zero outside the image),
// and the output columns of the tile are the contiguous (tap, c) columns of dW[n][tap][c].  For the stem (Cin = 8: one chunk per tap)
// all nine taps share one 128-column tile and one pass over G instead of nine.
template <int TN, int TC, bool COLS = false>
__device__ __forceinline__ void wgrad4_body(const WgradArgs& p, const int bid) {
    constexpr int ST = (TN + TC <= 128) ? 8 : 4;                  // ring depth: 64 KB (64+64: 8 x 8 KB, 128+128: 4 x 16 KB), 48 KB otherwise
    constexpr int PG = TN / 64, PX = TC / 64, PER = PG + PX;      // 1 KiB DMA pieces per wave and step
    constexpr int RG = 512 / TN, RX = 512 / TC;                   // tile rows per piece
    constexpr int NI = TN / 32, CI = TC / 32;                     // accumulator tiles per wave (waves 2 x 2)
    constexpr int STAGE = 32 * (TN + TC);                         // elements
    __shared__ __attribute__((aligned(1024))) uint16_t ring[ST * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wc = wave & 1;
    const int xcd = bid & 7, k_in = bid >> 3;
    const int zslice = xcd + 8 * (k_in / p.ntiles3), tile3 = k_in % p.ntiles3;
    if (zslice >= p.nslices3) return;            // padding workgroups of the last group of 8 slices (whole workgroup, before any barrier)
    const int ntile = tile3 / p.ctiles, ctile = tile3 - ntile * p.ctiles;
    const int n0 = ntile * TN, c0 = ctile * TC;
    const int m_begin = zslice * p.m_per_slice;
    const int m_end = min(p.M, m_begin + p.m_per_slice);
    const int nsteps = (max(m_end - m_begin, 0) + 31) / 32;
    const auto rx = MAKE_RSRC(p.x);
    const auto rg = MAKE_RSRC(p.g);
    // this wave's pieces: G pieces wave + 4 j (j < PG), X pieces wave + 4 j (j < PX); lane -> (row in piece, physical chunk)
    const int ncols = COLS ? 9 * p.Cin : p.Cin;                      // columns of the X operand = row length of one output row
    int gm[PG], xm[PX];
    unsigned goff[PG], xoff[PX];
    bool gcol[PG], xcol[PX];
    int xb[PX], xoy[PX], xox[PX], xkh[PX], xkw[PX], xch[PX];         // column form: pixel of the lane's row (carried), its tap and channel
#pragma unroll
    for (int j = 0; j < PG; ++j) {
        const int row = (wave + 4 * j) * RG + lane / (TN / 8);
        const int col = n0 + (((lane % (TN / 8)) ^ w4_swz<TN>(row)) << 3);
        gm[j] = m_begin + row;
        gcol[j] = col < p.N;
        goff[j] = (unsigned)((gm[j] * p.N + col) * 2);
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int row = (wave + 4 * j) * RX + lane / (TC / 8);
        const int col = c0 + (((lane % (TC / 8)) ^ w4_swz<TC>(row)) << 3);
        xm[j] = m_begin + row;
        xcol[j] = col < ncols;
        xoff[j] = (unsigned)((xm[j] * p.Cin + col) * 2);
        if (COLS) {
            const int tap = col / p.Cin, hw = p.Ho * p.Wo;
            xch[j] = col - tap * p.Cin;
            xkh[j] = tap / 3 - p.pad;
            xkw[j] = tap % 3 - p.pad;
            xb[j] = xm[j] / hw;
            const int r = xm[j] - xb[j] * hw;
            xoy[j] = r / p.Wo;
            xox[j] = r - xoy[j] * p.Wo;
        }
    }
    const unsigned gstep = (unsigned)(64 * p.N), xstep = (unsigned)(64 * p.Cin);       // bytes per 32 rows
    int issued = 0;
    auto issue_next = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)
        uint16_t* sg = ring + (issued & (ST - 1)) * STAGE;
        uint16_t* sx = sg + 32 * TN;
        ++issued;
#pragma unroll
        for (int j = 0; j < PG; ++j) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, W4_LDS(sg + (wave + 4 * j) * 512), 16, (gcol[j] && gm[j] < m_end) ? goff[j] : OOB_OFF, 0, 0, 0);
            gm[j] += 32;
            goff[j] += gstep;
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            unsigned off = (xcol[j] && xm[j] < m_end) ? xoff[j] : OOB_OFF;
            if (COLS) {
                const int iy = xoy[j] * p.stride + xkh[j], ix = xox[j] * p.stride + xkw[j];
                const bool in = xcol[j] && xm[j] < m_end && iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws;
                off = in ? (unsigned)((((xb[j] * p.Hs + iy) * p.Ws + ix) * p.Cin + xch[j]) * 2) : OOB_OFF;
                xox[j] += 32;                                 // next step: 32 output pixels further, with carries
                while (xox[j] >= p.Wo) {
                    xox[j] -= p.Wo;
                    if (++xoy[j] == p.Ho) {
                        xoy[j] = 0;
                        ++xb[j];
                    }
                }
            }
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, W4_LDS(sx + (wave + 4 * j) * 512), 16, off, 0, 0, 0);
            xm[j] += 32;
            xoff[j] += xstep;
        }
#endif
    };
    f32x4 acc[NI][CI], accb[NI];
#pragma unroll
    for (int a = 0; a < NI; ++a) {
        accb[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < CI; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = p.bias_part && ctile == 0 && wc == 0;          // wave-uniform
    const bf16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
#pragma unroll
    for (int j = 0; j < ST - 1; ++j) issue_next();       // steps beyond the slice fetch zero tiles: the counts stay uniform
    for (int s = 0; s < nsteps; ++s) {
        w4_wait_vm<(ST - 2) * PER>();                    // this wave's pieces of step s have landed ...
        __builtin_amdgcn_s_barrier();                    // ... everyone's have, and everyone is done with stage (s - 1) % ST
        issue_next();
        const uint16_t* sg = ring + (s & (ST - 1)) * STAGE;
        const uint16_t* sx = sg + 32 * TN;
        s16x4 gl[NI], gh[NI], xl[CI], xh[CI];
#pragma unroll
        for (int a = 0; a < NI; ++a) w4_frag<TN>(sg, wn * (TN / 2) + a * 16, lane, gl[a], gh[a]);
#pragma unroll
        for (int b = 0; b < CI; ++b) w4_frag<TC>(sx, wc * (TC / 2) + b * 16, lane, xl[b], xh[b]);
#pragma unroll
        for (int a = 0; a < NI; a += 2) ring_fence4(gl[a], gh[a], gl[a + 1], gh[a + 1]);
#pragma unroll
        for (int b = 0; b < CI; b += 2) ring_fence4(xl[b], xh[b], xl[b + 1], xh[b + 1]);
        bf16x8 gf[NI], xf[CI];
#pragma unroll
        for (int a = 0; a < NI; ++a) gf[a] = ring_join(gl[a], gh[a]);
#pragma unroll
        for (int b = 0; b < CI; ++b) xf[b] = ring_join(xl[b], xh[b]);
#pragma unroll
        for (int a = 0; a < NI; ++a)
#pragma unroll
            for (int b = 0; b < CI; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[a], xf[b], acc[a][b], 0, 0, 0);
        if (do_bias) {
#pragma unroll
            for (int a = 0; a < NI; ++a) accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[a], ones, accb[a], 0, 0, 0);
        }
    }
    w4_wait_vm<0>();                                     // the run-ahead zero tiles must have landed before the LDS is released
    float* dst = p.part + (size_t)zslice * p.N * ncols;
#pragma unroll
    for (int a = 0; a < NI; ++a) {
        const int n = n0 + wn * (TN / 2) + a * 16 + (lane >> 4) * 4;
#pragma unroll
        for (int b = 0; b < CI; ++b) {
            const int c = c0 + wc * (TC / 2) + b * 16 + (lane & 15);
            if (c < ncols) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < p.N) dst[(size_t)(n + r) * ncols + c] = acc[a][b][r];
            }
        }
        if (do_bias && (lane & 15) == 0) {               // every column of the ones product holds the column sums of G
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < p.N) p.bias_part[(size_t)zslice * p.N + n + r] = accb[a][r];
        }
    }
}
template <int TN, int TC, bool COLS = false>
__global__ void __launch_bounds__(256, 2) k_wgrad4(WgradArgs p) { wgrad4_body<TN, TC, COLS>(p, (int)blockIdx.x); }
// grouped form (round 4): the weight gradients of all the conv layers of one exchange-unit level in ONE launch; every member's block
// range starts at a multiple of 8, so (local id & 7) is still the XCD a slice is dealt to
struct WgradGroup {
    WgradArgs a[PK_GROUP_MAX];
    int first[PK_GROUP_MAX + 1];
    int n;
};
template <int TN, int TC, bool COLS>
__global__ void __launch_bounds__(256, 2) k_wgrad4g(WgradGroup g) {
    const int L = (int)blockIdx.x;
    PK_GROUP_MEMBER(i, g.first, g.n, L);
    wgrad4_body<TN, TC, COLS>(g.a[i], L - g.first[i]);
}

// k_wgrad4w: the single-tap kernel for operands whose rows are GATHERED through the 7x7 window partition and / or SCALED per sample
// (unfused attention: qkv weight gradient reads LN(x) in window order, proj reads dy in window order times the DropPath scale;
// unfused MLP: fc2 reads dy times the scale).  Loading the int32 row map would put a dependent global load in front of every DMA
// issue, so the map is RECOMPUTED: the caller passes the token grid (B, Hs, Ws) with the map (which must be nnops.window_rowmap of
// that grid; M = B * ceil(Hs/7) * ceil(Ws/7) * 49 is checked), and every DMA lane carries (token in window, window x, window y,
// sample) from step to step.  Row scales travel with the data: one 4-byte LDS-DMA per G piece fetches g_scale[sample] for the
// piece's rows into a per-stage slot (lane-linear, i.e. one copy per 16-byte chunk of the row), the fragments are scaled in
// registers after the transpose read (the bias gradient is the column sum of the SCALED rows, as in k_wgrad2).
struct WinPos { int t, wx, wy, b; };
__device__ __forceinline__ WinPos win_split(int m, int nw, int nh) {
    WinPos r;
    const int w = m / 49;
    r.t = m - 49 * w;
    const int q = w / nw;
    r.wx = w - q * nw;
    r.b = q / nh;
    r.wy = q - r.b * nh;
    return r;
}
__device__ __forceinline__ void win_advance(WinPos& r, int nw, int nh) {      // + 32 rows (< 49: at most one window further)
    r.t += 32;
    if (r.t >= 49) {
        r.t -= 49;
        if (++r.wx == nw) {
            r.wx = 0;
            if (++r.wy == nh) {
                r.wy = 0;
                ++r.b;
            }
        }
    }
}
__device__ __forceinline__ int win_row(const WinPos& r, int H, int W) {       // pixel row of the token, -1 = zero-pad token
    const int ty = (r.t * 37) >> 8, tx = r.t - 7 * ty;                         // t / 7, t % 7 for t < 49
    const int y = r.wy * 7 + ty, x = r.wx * 7 + tx;
    return (y < H && x < W) ? (r.b * H + y) * W + x : -1;
}
__device__ __forceinline__ float ring_f32(const float* a) {
    float v;
    asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)a) : "memory");
    return v;
}
__device__ __forceinline__ s16x4 scale_bf16x4(const s16x4& v, const float* sc) {
    const uint32_t lo = pack_bf16x2(__uint_as_float((uint32_t)(uint16_t)v[0] << 16) * sc[0], __uint_as_float((uint32_t)(uint16_t)v[1] << 16) * sc[1]);
    const uint32_t hi = pack_bf16x2(__uint_as_float((uint32_t)(uint16_t)v[2] << 16) * sc[2], __uint_as_float((uint32_t)(uint16_t)v[3] << 16) * sc[3]);
    return (s16x4){(short)(lo & 0xffff), (short)(lo >> 16), (short)(hi & 0xffff), (short)(hi >> 16)};
}
// MODE: which of the three run-time variations this instantiation serves (they were uniform run-time flags tested for every DMA piece of
// every 32-row step; a step of the 128 x 128 tile was 445 instructions around 20 MFMAs): 0 = any (generic), 1 = A rows gathered through the
// window partition only (qkv weight gradient), 2 = G rows gathered + scaled per sample (proj), 3 = G rows scaled only (fc2 of the unfused MLP).
template <int TN, int TC, int MODE = 0>
__global__ void __launch_bounds__(256, 2) k_wgrad4w(WgradArgs p) {
    constexpr int ST = (TN + TC >= 256) ? 3 : 4;                  // ring <= 48 KB + <= 8 KB of row scales: two workgroups per CU
    constexpr int PG = TN / 64, PX = TC / 64, PER = 2 * PG + PX;  // DMA instructions per wave and step: data pieces + one scale piece per G piece
    constexpr int RG = 512 / TN, RX = 512 / TC;
    constexpr int NI = TN / 32, CI = TC / 32;
    constexpr int STAGE = 32 * (TN + TC), SCW = 4 * PG * 64;      // elements per stage; floats of row scales per stage
    __shared__ __attribute__((aligned(1024))) uint16_t ring[ST * STAGE];
    __shared__ __attribute__((aligned(1024))) float sS[ST * SCW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wc = wave & 1;
    const int xcd = blockIdx.x & 7, k_in = blockIdx.x >> 3;
    const int zslice = xcd + 8 * (k_in / p.ntiles3), tile3 = k_in % p.ntiles3;
    if (zslice >= p.nslices3) return;
    const int ntile = tile3 / p.ctiles, ctile = tile3 - ntile * p.ctiles;
    const int n0 = ntile * TN, c0 = ctile * TC;
    const int m_begin = zslice * p.m_per_slice;
    const int m_end = min(p.M, m_begin + p.m_per_slice);
    const int nsteps = (max(m_end - m_begin, 0) + 31) / 32;
    const bool gwin = MODE == 0 ? p.g_rowmap != nullptr : MODE == 2, xwin = MODE == 0 ? p.a_rowmap != nullptr : MODE == 1,
               scaled = MODE == 0 ? p.g_scale != nullptr : MODE >= 2;     // workgroup-uniform; compile-time in the specialised instantiations
    const int nw = (p.Ws + 6) / 7, nh = (p.Hs + 6) / 7;
    const auto rx = MAKE_RSRC(p.x);
    const auto rg = MAKE_RSRC(p.g);
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(scaled ? const_cast<float*>(p.g_scale) : (float*)const_cast<uint16_t*>(p.g), 0, 0x7ffffff0, 0x00020000);
    int gm[PG], xm[PX], gsb[PG], gsr[PG];
    unsigned gcb[PG], xcb[PX];                      // byte offset of the lane's chunk inside a source row
    bool gcol[PG], xcol[PX];
    WinPos gw[PG], xw[PX];
#pragma unroll
    for (int j = 0; j < PG; ++j) {
        const int row = (wave + 4 * j) * RG + lane / (TN / 8);
        const int col = n0 + (((lane % (TN / 8)) ^ w4_swz<TN>(row)) << 3);
        gm[j] = m_begin + row;
        gcol[j] = col < p.N;
        gcb[j] = (unsigned)(col * 2);
        gw[j] = gwin ? win_split(gm[j], nw, nh) : WinPos{0, 0, 0, 0};
        gsb[j] = scaled ? gm[j] / p.g_rows_per_sample : 0;
        gsr[j] = scaled ? gm[j] - gsb[j] * p.g_rows_per_sample : 0;
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int row = (wave + 4 * j) * RX + lane / (TC / 8);
        const int col = c0 + (((lane % (TC / 8)) ^ w4_swz<TC>(row)) << 3);
        xm[j] = m_begin + row;
        xcol[j] = col < p.Cin;
        xcb[j] = (unsigned)(col * 2);
        xw[j] = xwin ? win_split(xm[j], nw, nh) : WinPos{0, 0, 0, 0};
    }
    int wr = 0;
    auto issue_next = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)
        uint16_t* sg = ring + wr * STAGE;
        uint16_t* sx = sg + 32 * TN;
        float* ss = sS + wr * SCW;
        wr = (wr + 1 == ST) ? 0 : wr + 1;
#pragma unroll
        for (int j = 0; j < PG; ++j) {
            const int src = gwin ? win_row(gw[j], p.Hs, p.Ws) : gm[j];
            const bool live = gm[j] < m_end && src >= 0;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, W4_LDS(sg + (wave + 4 * j) * 512), 16,
                                                     (live && gcol[j]) ? (unsigned)(src * p.N * 2) + gcb[j] : OOB_OFF, 0, 0, 0);
            const int sample = gwin ? gw[j].b : gsb[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, W4_LDS(ss + (wave + 4 * j) * 64), 4, (live && scaled) ? (unsigned)(sample * 4) : OOB_OFF, 0, 0, 0);
            gm[j] += 32;
            if (gwin) win_advance(gw[j], nw, nh);
            else if (scaled) {
                gsr[j] += 32;
                while (gsr[j] >= p.g_rows_per_sample) {
                    gsr[j] -= p.g_rows_per_sample;
                    ++gsb[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const int src = xwin ? win_row(xw[j], p.Hs, p.Ws) : xm[j];
            const bool live = xm[j] < m_end && src >= 0 && xcol[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, W4_LDS(sx + (wave + 4 * j) * 512), 16, live ? (unsigned)(src * p.Cin * 2) + xcb[j] : OOB_OFF, 0, 0, 0);
            xm[j] += 32;
            if (xwin) win_advance(xw[j], nw, nh);
        }
#endif
    };
    f32x4 acc[NI][CI], accb[NI];
#pragma unroll
    for (int a = 0; a < NI; ++a) {
        accb[a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < CI; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = p.bias_part && ctile == 0 && wc == 0;
    const bf16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
    // row scales of this lane's fragment rows 8 g .. 8 g + 7: piece = row / RG, one copy per chunk lane -> take the first
    int sidx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = 8 * (lane >> 4) + i;
        sidx[i] = (r / RG) * 64 + (r % RG) * (TN / 8);
    }
#pragma unroll
    for (int j = 0; j < ST - 1; ++j) issue_next();
    int rd = 0;
    for (int s = 0; s < nsteps; ++s) {
        w4_wait_vm<(ST - 2) * PER>();
        __builtin_amdgcn_s_barrier();
        issue_next();
        const uint16_t* sg = ring + rd * STAGE;
        const uint16_t* sx = sg + 32 * TN;
        const float* ss = sS + rd * SCW;
        rd = (rd + 1 == ST) ? 0 : rd + 1;
        s16x4 gl[NI], gh[NI], xl[CI], xh[CI];
        float sc[8];
#pragma unroll
        for (int a = 0; a < NI; ++a) w4_frag<TN>(sg, wn * (TN / 2) + a * 16, lane, gl[a], gh[a]);
#pragma unroll
        for (int b = 0; b < CI; ++b) w4_frag<TC>(sx, wc * (TC / 2) + b * 16, lane, xl[b], xh[b]);
        if (scaled) {
#pragma unroll
            for (int i = 0; i < 8; ++i) sc[i] = ring_f32(ss + sidx[i]);
        }
#pragma unroll
        for (int a = 0; a < NI; a += 2) ring_fence4(gl[a], gh[a], gl[a + 1], gh[a + 1]);
#pragma unroll
        for (int b = 0; b < CI; b += 2) ring_fence4(xl[b], xh[b], xl[b + 1], xh[b + 1]);
        if (scaled) {
            asm volatile("" : "+v"(sc[0]), "+v"(sc[1]), "+v"(sc[2]), "+v"(sc[3]), "+v"(sc[4]), "+v"(sc[5]), "+v"(sc[6]), "+v"(sc[7]));
#pragma unroll
            for (int a = 0; a < NI; ++a) {
                gl[a] = scale_bf16x4(gl[a], sc);
                gh[a] = scale_bf16x4(gh[a], sc + 4);
            }
        }
        bf16x8 gf[NI], xf[CI];
#pragma unroll
        for (int a = 0; a < NI; ++a) gf[a] = ring_join(gl[a], gh[a]);
#pragma unroll
        for (int b = 0; b < CI; ++b) xf[b] = ring_join(xl[b], xh[b]);
#pragma unroll
        for (int a = 0; a < NI; ++a)
#pragma unroll
            for (int b = 0; b < CI; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[a], xf[b], acc[a][b], 0, 0, 0);
        if (do_bias) {
#pragma unroll
            for (int a = 0; a < NI; ++a) accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[a], ones, accb[a], 0, 0, 0);
        }
    }
    w4_wait_vm<0>();
    float* dst = p.part + (size_t)zslice * p.N * p.Cin;
#pragma unroll
    for (int a = 0; a < NI; ++a) {
        const int n = n0 + wn * (TN / 2) + a * 16 + (lane >> 4) * 4;
#pragma unroll
        for (int b = 0; b < CI; ++b) {
            const int c = c0 + wc * (TC / 2) + b * 16 + (lane & 15);
            if (c < p.Cin) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < p.N) dst[(size_t)(n + r) * p.Cin + c] = acc[a][b][r];
            }
        }
        if (do_bias && (lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < p.N) p.bias_part[(size_t)zslice * p.N + n + r] = accb[a][r];
        }
    }
}

__global__ void __launch_bounds__(256, 2) k_wgrad4_3x3(WgradArgs p) {
    constexpr int W = 64, ST = 4, XR = 256;                                   // tile width, G stages, X ring rows
    __shared__ __attribute__((aligned(1024))) uint16_t sG[ST * 32 * W];       // 16 KB
    __shared__ __attribute__((aligned(1024))) uint16_t sX[XR * W];            // 32 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int xcd = blockIdx.x & 7, k_in = blockIdx.x >> 3;
    const int zslice = xcd + 8 * (k_in / p.ntiles3), tile3 = k_in % p.ntiles3;
    if (zslice >= p.nslices3) return;
    const int ntile = tile3 / p.ctiles, ctile = tile3 - ntile * p.ctiles;
    const int n0 = ntile * W, c0 = ctile * W;
    const int PW = p.Ws + 2, PH = p.Hs + 2, PP = PH * PW;
    const int B = p.M / (p.Hs * p.Ws), MP = B * PP;                          // stride 1, pad 1: Ho = Hs, Wo = Ws
    const int p_begin = zslice * p.m_per_slice;                              // multiple of 32
    const int p_end = min(MP, p_begin + p.m_per_slice);
    const int nsteps = (max(p_end - p_begin, 0) + 31) / 32;
    const auto rx = MAKE_RSRC(p.x);
    const auto rg = MAKE_RSRC(p.g);
    // DMA roles: 8 rows per 1 KiB piece, piece `wave` of every 32-row block; lane -> (row in piece, physical chunk).  The padded pixel
    // of the lane's row is carried as (b, py, px) and advanced by 32 per block.
    const int prow = 8 * wave + (lane >> 3);
    struct Pix { int b, py, px; };
    auto split = [&](int q) {                     // q >= -PP
        Pix r;
        const int qq = q + PP;
        r.b = qq / PP - 1;
        const int rem = qq - (r.b + 1) * PP;
        r.py = rem / PW;
        r.px = rem - r.py * PW;
        return r;
    };
    auto advance = [&](Pix& r) {
        r.px += 32;
        while (r.px >= PW) {
            r.px -= PW;
            if (++r.py == PH) {
                r.py = 0;
                ++r.b;
            }
        }
    };
    auto interior = [&](const Pix& r) { return r.b >= 0 && r.b < B && r.py >= 1 && r.py <= p.Hs && r.px >= 1 && r.px <= p.Ws; };
    Pix gp = split(p_begin + prow);
    int gq = p_begin + prow;                                                  // padded pixel of the lane's G row
    const int gcolumn = n0 + (((lane & 7) ^ w4_swz<W>(prow)) << 3);
    const bool gcol = gcolumn < p.N;
    int xq = p_begin - 64 + prow;                                             // X runs ahead: the buffer is filled from p_begin - 64
    Pix xp = split(xq);
    const int xcolumn = c0 + (((lane & 7) ^ w4_swz<W>(xq & (XR - 1))) << 3);  // (ring row bits 0, 1, 3 never change: +32 per block)
    const bool xcol = xcolumn < p.Cin;
    int g_issued = 0;
    auto issue_x = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)
        const bool ok = xcol && interior(xp);
        const unsigned off = ok ? (unsigned)((((xp.b * p.Hs + xp.py - 1) * p.Ws + xp.px - 1) * p.Cin + xcolumn) * 2) : OOB_OFF;
        const int base_row = (xq - (lane >> 3)) & (XR - 1);                   // wave-uniform: first ring row of this piece
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, W4_LDS(sX + base_row * W), 16, off, 0, 0, 0);
        xq += 32;
        advance(xp);
#endif
    };
    auto issue_g = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)
        const bool ok = gcol && gq < p_end && interior(gp);
        const unsigned off = ok ? (unsigned)((((gp.b * p.Hs + gp.py - 1) * p.Ws + gp.px - 1) * p.N + gcolumn) * 2) : OOB_OFF;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, W4_LDS(sG + (g_issued & (ST - 1)) * 32 * W + 8 * wave * W), 16, off, 0, 0, 0);
        ++g_issued;
        gq += 32;
        advance(gp);
#endif
    };
    // fragment addresses of the nine taps (bytes inside sX), advanced by 32 rows = 4 096 bytes per step (swizzle bits unchanged)
    const int g4 = lane >> 4, i4 = lane & 15, q4 = i4 >> 2, pq4 = i4 & 3;
    int alo[9], ahi[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int r0 = p_begin + (t / 3 - 1) * PW + (t % 3 - 1) + 8 * g4 + q4 + XR;          // >= 0: p_begin >= 0, halo < 256
        alo[t] = 2 * w4_elem<W>(r0 & (XR - 1), 16 * wave, pq4);
        ahi[t] = 2 * w4_elem<W>((r0 + 4) & (XR - 1), 16 * wave, pq4);
    }
    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[t][a] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // prologue: X blocks p_begin - 64 .. p_begin + 63, then three (G, X) steps in flight
    issue_x();
    issue_x();
    issue_x();
    issue_x();
#pragma unroll
    for (int j = 0; j < ST - 1; ++j) {
        issue_g();
        issue_x();
    }
    const char* sXb = reinterpret_cast<const char*>(sX);
    for (int s = 0; s < nsteps; ++s) {
        w4_wait_vm<(ST - 2) * 2>();          // landed: G of step s and X up to p0 + 95 (taps reach p0 + 31 + PW + 1 <= p0 + 82)
        __builtin_amdgcn_s_barrier();        // everyone is done with step s - 1: its G stage and the X rows below p0 - 64 may be overwritten
        issue_g();
        issue_x();
        const uint16_t* sg = sG + (s & (ST - 1)) * 32 * W;
        // three groups of reads (G + taps 0..1 | taps 2..5 | taps 6..8); each group is in flight under the previous group's MFMAs
        s16x4 gl[4], gh[4], xl[9], xh[9];
#pragma unroll
        for (int a = 0; a < 4; ++a) w4_frag<W>(sg, a * 16, lane, gl[a], gh[a]);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t == 2) {
                ring_fence(gl[0], gh[0], gl[1], gh[1], gl[2], gh[2], gl[3], gh[3]);
                ring_fence4(xl[0], xh[0], xl[1], xh[1]);
            }
            if (t == 6) ring_fence(xl[2], xh[2], xl[3], xh[3], xl[4], xh[4], xl[5], xh[5]);
            xl[t] = ring_tr(reinterpret_cast<const uint16_t*>(sXb + alo[t]));
            xh[t] = ring_tr(reinterpret_cast<const uint16_t*>(sXb + ahi[t]));
            alo[t] = (alo[t] + 32 * W * 2) & (XR * W * 2 - 1);
            ahi[t] = (ahi[t] + 32 * W * 2) & (XR * W * 2 - 1);
            if (t == 5 || t == 8) {        // MFMAs of the group fenced before this one was issued
                const int t0 = (t == 5) ? 0 : 2, t1 = (t == 5) ? 2 : 6;
#pragma unroll
                for (int u = t0; u < t1; ++u) {
                    const bf16x8 xf = ring_join(xl[u], xh[u]);
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        acc[u][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring_join(gl[a], gh[a]), xf, acc[u][a], 0, 0, 0);
                }
            }
        }
        ring_fence4(xl[6], xh[6], xl[7], xh[7]);
        asm volatile("" : "+v"(xl[8]), "+v"(xh[8]));       // (the fence above waited for all of them; this pins tap 8 behind it)
#pragma unroll
        for (int u = 6; u < 9; ++u) {
            const bf16x8 xf = ring_join(xl[u], xh[u]);
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[u][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring_join(gl[a], gh[a]), xf, acc[u][a], 0, 0, 0);
        }
    }
    w4_wait_vm<0>();
    float* dst = p.part + (size_t)zslice * p.N * 9 * p.Cin;
    const int c = c0 + 16 * wave + (lane & 15);
    if (c < p.Cin) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int n = n0 + a * 16 + (lane >> 4) * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < p.N) dst[((size_t)(n + r) * 9 + t) * p.Cin + c] = acc[t][a][r];
            }
    }
}
// out[...] = sum_s part[s][n][t][c]; layout 0: [N][T][Cin]; layout 1: OIHW = [N][Cin][T] (reference conv weight layout).
// Block = 16 elements x 16 slice-lanes (lane r sums slices s = r mod 16, fixed-order combine): short dependency chains
// even with hundreds of slices, still deterministic.
__global__ void __launch_bounds__(256) k_wgrad_reduce(const float* __restrict__ part, float* __restrict__ out, int S, int N, int T,
                                                      int Cin, int layout, const float* __restrict__ bias_part, float* __restrict__ dbias,
                                                      int n_bias, int w_blocks) {
    __shared__ float sh[16][17];
    const int col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    if ((int)blockIdx.x >= w_blocks) {          // trailing blocks: bias-gradient slabs [S][N] -> dbias[0..n_bias)
        const int n = (blockIdx.x - w_blocks) * 16 + col;
        float s = 0.f;
        if (n < n_bias)
            for (int k = rl; k < S; k += 16) s += bias_part[(size_t)k * N + n];
        sh[rl][col] = s;
        __syncthreads();
        if (rl != 0 || n >= n_bias) return;
        s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += sh[r][col];
        dbias[n] = s;
        return;
    }
    const int total = N * T * Cin;
    const int i = blockIdx.x * 16 + col;
    float s = 0.f;
    if (i < total)
        for (int k = rl; k < S; k += 16) s += part[(size_t)k * total + i];
    sh[rl][col] = s;
    __syncthreads();
    if (rl != 0 || i >= total) return;
    s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += sh[r][col];
    if (layout == 0) out[i] = s;
    else {
        const int c = i % Cin, t = (i / Cin) % T, n = i / (Cin * T);
        out[((size_t)n * Cin + c) * T + t] = s;
    }
}

// Deferred parameter-gradient reductions.  Nothing in backward reads a parameter gradient, yet every split-M weight
// gradient, LayerNorm dgamma/dbeta and rel-pos-bias gradient ended with its own small slab-reduce launch in the middle of
// the data-gradient chain (~360 of the ~2 000 launches per step, each 6-12 us plus the dependency bubble around it).  With
// dw/dgamma/dtable == NULL the producers only write their slabs; ONE table-driven launch at the end of backward reduces
// them all:   out[index(i)] = sum_{s < S} part[s * slab_stride + i],  i < K
//   layout 0: index(i) = i * out_stride;   layout 1 (conv OIHW): i = (n*T + t)*Cin + c  ->  (n*Cin + c)*T + t;
//   layout 2 (2-D slice): i = a*Cin + b  ->  a*T + b*out_stride  (a column block of a wider row-major matrix).
// Fixed-order combine (deterministic).
struct ReduceDesc { const float* part; float* out; int64_t slab_stride; int S, K, layout, N, T, Cin, out_stride, pad_; };
// Block = 64 outputs (16 groups of 4 consecutive) x 16 slab-lanes: 16-byte loads, 256 contiguous bytes per slab row and block
// (the first version read 64-byte pieces and ran at a quarter of the HBM rate: 1.17 ms per step for ~1.5 GB of slabs.  Measured and
// dropped in round 2: 1 KiB contiguous per slab row x 4 slab-lanes with four rows in flight per lane -- 1 310 us instead of 686 us;
// and, for the 3x3 weights whose OIHW destination is written one float every 36 bytes, a block per (n, 64 channels, nine taps) with
// the destination run transposed through LDS and written contiguously -- step 18.3 -> 18.56 ms.  Round 3: four independent loads per
// thread and round (rows k, k+16, k+32, k+48) -- unchanged, 637 us for the step's 2.29 GB = 3.6 TB/s; four 64-output groups per workgroup
// (45 000 workgroups instead of 180 000, four loads in flight per thread) -- 1 072 us.)
__global__ void __launch_bounds__(256) k_reduce_many(const ReduceDesc* __restrict__ desc, const int* __restrict__ blk_desc,
                                                     const int* __restrict__ blk_first) {
    __shared__ float4 sh[16][17];
    const ReduceDesc d = desc[blk_desc[blockIdx.x]];
    const int col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int i = ((blockIdx.x - blk_first[blockIdx.x]) * 16 + col) * 4;
    const bool vec = ((d.K | (int)d.slab_stride) & 3) == 0 && (((uintptr_t)d.part) & 15) == 0;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < d.K) {
        if (vec) {
            for (int k = rl; k < d.S; k += 16) {
                const float4 v = *reinterpret_cast<const float4*>(d.part + (size_t)k * d.slab_stride + i);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        } else {
            for (int k = rl; k < d.S; k += 16) {
                const float* p = d.part + (size_t)k * d.slab_stride + i;
                s.x += p[0];
                if (i + 1 < d.K) s.y += p[1];
                if (i + 2 < d.K) s.z += p[2];
                if (i + 3 < d.K) s.w += p[3];
            }
        }
    }
    sh[rl][col] = s;
    __syncthreads();
    if (rl != 0 || i >= d.K) return;
    s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float4 v = sh[r][col];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float o4[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ij = i + j;
        if (ij >= d.K) break;
        if (d.layout == 0) d.out[(size_t)ij * d.out_stride] = o4[j];
        else if (d.layout == 2) d.out[(size_t)(ij / d.Cin) * d.T + (size_t)(ij % d.Cin) * d.out_stride] = o4[j];   // 2-D: [a][b < Cin] -> a*T + b*out_stride
        else {
            const int c = ij % d.Cin, t = (ij / d.Cin) % d.T, n = ij / (d.Cin * d.T);
            d.out[((size_t)n * d.Cin + c) * d.T + t] = o4[j];
        }
    }
}
extern "C" int pk_reduce_many_cols(void) { return 64; }     /* outputs per block: n_blocks = sum over rows of ceil(K / this) */
extern "C" int pk_reduce_many(const void* desc_table, const int* block_desc, const int* block_first, int n_blocks, void* stream) {
    PK_REQUIRE(desc_table && block_desc && block_first && n_blocks > 0, "pk_reduce_many: bad argument");
    hipLaunchKernelGGL(k_reduce_many, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, (const ReduceDesc*)desc_table, block_desc, block_first);
    return pk_launch_status("pk_reduce_many");
}

// ================================================================================================ routing
// Which kernel, tile, slice count and grid a weight gradient gets is decided in wgrad_route (wgrad_group_route for the grouped form) and
// nowhere else: pk_wgrad_bf16 launches from the route, pk_wgrad_slices returns its S, and the bias slabs start S weight slabs into the
// workspace.  flags: bit 0 = a_rowmap, 1 = g_rowmap, 2 = g_scale.
enum WgradKernel {
    WG_WGRAD2,         // k_wgrad2: register-staged, whatever the streaming kernels do not take (1x1 stride 2, gathered rows without a token grid)
    WG_WGRAD3,         // k_wgrad3: 3x3 with N and Cin multiples of 256 (the fusion head)
    WG_WGRAD4,         // k_wgrad4: single tap (linear layers, 1x1 stride-1 convolutions)
    WG_WGRAD4_COLS,    // k_wgrad4, column form: 3x3 convolutions that k_wgrad4_3x3 does not take (stride 2, wide maps)
    WG_WGRAD4W,        // k_wgrad4w: single tap with window-gathered and / or scaled rows
    WG_WGRAD4_3X3      // k_wgrad4_3x3: 3x3 stride 1, all nine taps in one pass
};
struct WgradRoute {
    WgradKernel kernel;
    int mode, tn, tc;                                // k_wgrad4w: its MODE (which gather / scale paths are compiled in); output tile
    int S, rows;                                     // M-slices = fp32 slabs in the workspace; contraction length: M, or the padded pixels of k_wgrad4_3x3
    int ctiles, ntiles3, nslices3, m_per_slice;      // the WgradArgs fields of the same names
    dim3 grid, block;
    int lds;                                         // dynamic LDS bytes
};
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

static WgradKernel wgrad_kernel(int N, int Cin, int ksize, int stride, int Hs, int Ws, int flags) {
    const bool wide = ksize == 3 && (N % 256) == 0 && (Cin % 256) == 0;
    const WgradKernel not_streaming = wide ? WG_WGRAD3 : WG_WGRAD2;
    if (flags)         // gathered / scaled rows: linear form; a row map needs the token grid it is the window partition of
        return (ksize != 1 || stride != 1 || ((flags & 3) && (Hs <= 0 || Ws <= 0))) ? not_streaming : WG_WGRAD4W;
    if (ksize == 1 && stride == 1) return WG_WGRAD4;
    if (ksize != 3 || wide) return not_streaming;
    return (stride == 1 && Ws >= 1 && Ws <= 48) ? WG_WGRAD4_3X3 : WG_WGRAD4_COLS;
}

// k_wgrad2 output tile (TN x TC): 64 x 64 or 128 x 128.  Measured and dropped: a 256 x 128 tile (128 x 64 per wave, as in k_igemm2)
// is slower here (head conv 716 us vs 523 us) -- the weight-gradient kernel is bound by its global loads (46 % of the wave
// cycles parked on s_waitcnt) and the larger tile drops it from 3 to 2 waves per SIMD; 64 pixel rows per step instead of 32
// (more bytes in flight, half the barriers) costs occupancy as well: 734 us on the 128 tile, +0.4 ms per step on the 64 tile.
// What did help the 128 tile: all-VGPR accumulators at 4 waves per SIMD (527 -> 492 us).
static inline int wgrad2_tile(int N, int Cin) { return (N >= 128 && Cin >= 128) ? 128 : 64; }
static int wgrad2_slices(int M, int N, int Cin, int T) {
    // enough workgroups to fill 256 CUs several times over (>= 2048), but no slice shorter than 256 rows
    constexpr int target = 2048;
    // (shorter slices for the low-resolution branches were measured: 64-row slices cost +1.3 ms per step in slab traffic; longer ones
    // are slower as well -- 512 / 1 024 rows: +0.35 / +1.8 ms per step -- each k_wgrad2 workgroup is bound by its own load latency)
    constexpr int min_rows = 256;
    const int t = wgrad2_tile(N, Cin), tiles = ceil_div(N, t) * ceil_div(Cin, t) * T;
    int s = ceil_div(target, tiles);
    const int max_s = ceil_div(M, min_rows);
    if (s > max_s) s = max_s;
    return s < 1 ? 1 : (s > 512 ? 512 : s);
}
static int wgrad3_slices(int M, int N, int Cin) {
    // one 512-thread workgroup per CU (128 KB LDS ring): ~one round of equal-sized workgroups over the 256 CUs, in whole groups of
    // 8 slices (one slice per XCD and group)
    constexpr int wide_target = 256;
    const int tiles3 = (N / 256) * (Cin / 256) * 9;
    int s3 = wide_target / tiles3 / 8 * 8;
    if (s3 < 8) s3 = 8;
    const int max3 = (M + 1023) / 1024;
    if (s3 > max3) s3 = max3;
    return s3 < 1 ? 1 : s3;
}

// Pure: no HIP call.  Sizes must be positive (pk_wgrad_bf16 and pk_wgrad_slices check that first).
static WgradRoute wgrad_route(int M, int N, int Cin, int ksize, int stride, int Hs, int Ws, int flags) {
    WgradRoute r{};
    const int T = ksize * ksize;
    r.kernel = wgrad_kernel(N, Cin, ksize, stride, Hs, Ws, flags);
    r.rows = M; r.block = dim3(256);
    if (r.kernel == WG_WGRAD3) {
        r.tn = r.tc = 256; r.S = r.nslices3 = wgrad3_slices(M, N, Cin);
        r.m_per_slice = (ceil_div(M, r.S) + 63) / 64 * 64;
        r.ctiles = Cin / 256; r.ntiles3 = (N / 256) * r.ctiles;
        r.grid = dim3(8 * ((r.S + 7) / 8) * 9 * r.ntiles3); r.block = dim3(512); r.lds = W3_STAGES * 2 * W3_ROWS * 256 * 2;
    } else if (r.kernel == WG_WGRAD2) {
        r.tn = r.tc = wgrad2_tile(N, Cin); r.S = wgrad2_slices(M, N, Cin, T);
        r.m_per_slice = (ceil_div(M, r.S) + 63) / 64 * 64;
        r.ctiles = ceil_div(Cin, r.tc);
        r.grid = dim3(ceil_div(N, r.tn) * r.ctiles, T, r.S);
        if (T == 9) {          // nine taps: a flat grid, dealt to the XCDs slice by slice
            r.ntiles3 = r.grid.x; r.nslices3 = r.S;
            r.grid = dim3(8 * ((r.S + 7) / 8) * 9 * r.ntiles3);
        }
    } else {
        // the streaming kernels.  Two workgroups per CU (single tap) / one (3x3: nine accumulator sets), slices of >= 512 rows: against 256
        // the step is unchanged (17.3 / 17.6 ms on two boxes either way) and the slabs of the low-resolution branches halve (k_reduce_many
        // 653 -> 570 us isolated); 1 024 rows starve the small launches of workgroups (step + 0.6 ms)
        constexpr int t1 = 512, t9 = 256, min_rows = 512;
        const bool nine = r.kernel == WG_WGRAD4_3X3, cols = r.kernel == WG_WGRAD4_COLS;
        r.tn = (nine || N <= 64) ? 64 : 128;
        r.tc = (nine || (!cols && Cin <= 64)) ? 64 : 128;         // column form: 9 * Cin >= 72 columns
        if (nine) r.rows = (M / (Hs * Ws)) * (Hs + 2) * (Ws + 2);          // M = B * Hs * Ws
        r.ctiles = ceil_div(cols ? 9 * Cin : Cin, r.tc); r.ntiles3 = ceil_div(N, r.tn) * r.ctiles;
        r.S = ceil_div(nine ? t9 : t1, r.ntiles3);
        const int max_s = ceil_div(r.rows, min_rows);
        r.S = r.nslices3 = r.S > max_s ? (max_s < 1 ? 1 : max_s) : r.S;          // (ceil_div of positive counts: r.S >= 1)
        r.m_per_slice = (ceil_div(r.rows, r.S) + 31) / 32 * 32;
        r.grid = dim3(8 * ((r.S + 7) / 8) * r.ntiles3);
        if (r.kernel == WG_WGRAD4W) r.mode = flags == 1 ? 1 : (flags == 6 ? 2 : (flags == 4 ? 3 : 0));          // x gathered / g gathered and scaled / g scaled / general
    }
    return r;
}
extern "C" int pk_wgrad_slices(int M, int N, int Cin, int ksize, int stride, int Hs, int Ws, int flags) {
    if (M <= 0 || N <= 0 || Cin <= 0 || ksize <= 0) return 0;          // (a size query must not divide by a zero tile count)
    return wgrad_route(M, N, Cin, ksize, stride, Hs, Ws, flags).S;
}

// ---- grouped weight gradients (slabs only; the caller reduces them with pk_reduce_many).  Two member kinds: 1x1 stride-1 convs (single
// tap, 64 x 64 tiles) and 3x3 stride-2 convs (column form, 64 x 128 tiles); one fixed tile shape per kind so that one launch serves all.
static inline int wgrad_group_kind(int ksize, int stride) { return (ksize == 1 && stride == 1) ? 1 : ((ksize == 3 && stride == 2) ? 3 : 0); }
struct WgradGroupRoute { int kind, tn, tc, S, ctiles, ntiles3, m_per_slice, blocks; };          // kind 0 (neither): S = 0
static WgradGroupRoute wgrad_group_route(int M, int N, int Cin, int ksize, int stride) {
    WgradGroupRoute r{};
    r.kind = wgrad_group_kind(ksize, stride);
    if (!r.kind) return r;
    r.tn = 64; r.tc = r.kind == 3 ? 128 : 64;
    r.ctiles = ceil_div(r.kind == 3 ? 9 * Cin : Cin, r.tc); r.ntiles3 = ceil_div(N, r.tn) * r.ctiles;
    r.S = ceil_div(256, r.ntiles3);                    // ~one round of workgroups per member; slices of >= 512 rows
    const int max_s = ceil_div(M, 512);
    r.S = r.S > max_s ? (max_s < 1 ? 1 : max_s) : r.S;
    r.m_per_slice = (ceil_div(M, r.S) + 31) / 32 * 32;
    r.blocks = 8 * ((r.S + 7) / 8) * r.ntiles3;          // a multiple of 8 per member: see k_wgrad4g
    return r;
}
extern "C" int pk_wgrad_group_slices(int M, int N, int Cin, int ksize, int stride) { return wgrad_group_route(M, N, Cin, ksize, stride).S; }
extern "C" int pk_wgrad_group(const PkWgradDesc* d, int n, void* stream) {
    PK_REQUIRE(d && n > 0 && n <= PK_GROUP_MAX, "pk_wgrad_group: 1..%d members, got %d", PK_GROUP_MAX, n);
    WgradGroup g{};
    const int kind = wgrad_group_kind(d[0].ksize, d[0].stride);
    PK_SUPPORTED(kind != 0, "pk_wgrad_group: 1x1 stride-1 or 3x3 stride-2 convolutions only");
    int total = 0;
    for (int i = 0; i < n; ++i) {
        const PkWgradDesc& c = d[i];
        PK_REQUIRE(c.x && c.grad_out && c.workspace, "pk_wgrad_group: null pointer");
        PK_REQUIRE(wgrad_group_kind(c.ksize, c.stride) == kind, "pk_wgrad_group: members must be of one kind");
        const int M = c.B * c.Ho * c.Wo;
        PK_REQUIRE(M > 0 && c.N > 0 && c.Cin > 0 && c.Hs > 0 && c.Ws > 0, "pk_wgrad_group: bad sizes");
        PK_SUPPORTED((c.Cin & 7) == 0 && (c.N & 7) == 0, "pk_wgrad_group: Cin=%d and N=%d must be multiples of 8", c.Cin, c.N);
        PK_REQUIRE((int64_t)M * c.N < 0x3fffffffLL && (int64_t)c.B * c.Hs * c.Ws * c.Cin < 0x3fffffffLL, "pk_wgrad_group: tensor too large");
        PK_REQUIRE(kind == 3 || (c.Ho == c.Hs && c.Wo == c.Ws), "pk_wgrad_group: stride-1 geometry");
        const WgradGroupRoute r = wgrad_group_route(M, c.N, c.Cin, c.ksize, c.stride);
        WgradArgs& a = g.a[i];
        a.x = (const uint16_t*)c.x; a.g = (const uint16_t*)c.grad_out; a.part = c.workspace; a.g_rows_per_sample = 1;
        a.M = M; a.N = c.N; a.Cin = c.Cin; a.T = c.ksize * c.ksize; a.Hs = c.Hs; a.Ws = c.Ws; a.Ho = c.Ho; a.Wo = c.Wo; a.stride = c.stride;
        a.pad = c.ksize / 2;
        a.ctiles = r.ctiles; a.ntiles3 = r.ntiles3; a.nslices3 = r.S; a.m_per_slice = r.m_per_slice;
        g.first[i] = total;
        total += r.blocks;
    }
    g.first[n] = total;
    g.n = n;
    hipStream_t st = (hipStream_t)stream;
    if (kind == 3) hipLaunchKernelGGL((k_wgrad4g<64, 128, true>), dim3((unsigned)total), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((k_wgrad4g<64, 64, false>), dim3((unsigned)total), dim3(256), 0, st, g);
    return pk_launch_status("pk_wgrad_group");
}

static constexpr int wgrad_key(int kernel, int tn, int tc, int mode) { return ((kernel * 1000 + tn) * 1000 + tc) * 10 + mode; }
#define WGRAD_CASE(K, TN, TC, MODE, ...) case wgrad_key(K, TN, TC, MODE): hipLaunchKernelGGL(__VA_ARGS__, r.grid, r.block, r.lds, st, a); break;
#define WGRAD4W_CASES(TN, TC)                                                                                              \
    WGRAD_CASE(WG_WGRAD4W, TN, TC, 0, (k_wgrad4w<TN, TC, 0>)) WGRAD_CASE(WG_WGRAD4W, TN, TC, 1, (k_wgrad4w<TN, TC, 1>)) \
    WGRAD_CASE(WG_WGRAD4W, TN, TC, 2, (k_wgrad4w<TN, TC, 2>)) WGRAD_CASE(WG_WGRAD4W, TN, TC, 3, (k_wgrad4w<TN, TC, 3>))

extern "C" int pk_wgrad_bf16(const void* x, const void* grad_out, float* workspace, float* dw, float* dbias, int n_bias, const int32_t* a_rowmap,
                             const int32_t* g_rowmap, const float* g_scale, int g_rows_per_sample, int M, int N, int Cin, int ksize, int stride,
                             int B, int Hs, int Ws, int Ho, int Wo, int out_layout, void* stream) {
    PK_REQUIRE(x && grad_out && workspace, "pk_wgrad_bf16: null pointer");
    PK_REQUIRE(M > 0 && N > 0 && Cin > 0 && (ksize == 1 || ksize == 3), "pk_wgrad_bf16: bad sizes");
    PK_SUPPORTED((Cin & 7) == 0 && (N & 7) == 0, "pk_wgrad_bf16: Cin=%d and N=%d must be multiples of 8", Cin, N);
    const bool linear = (Ho == 0);
    if (!linear) PK_REQUIRE(M == B * Ho * Wo && (int64_t)B * Hs * Ws * Cin < 0x7fffffffLL, "pk_wgrad_bf16: geometry");
    PK_REQUIRE(linear || (!a_rowmap && !g_rowmap), "pk_wgrad_bf16: row maps are for the linear form only");
    PK_REQUIRE(!g_scale || g_rows_per_sample > 0, "pk_wgrad_bf16: g_scale needs g_rows_per_sample");
    const WgradRoute r = wgrad_route(M, N, Cin, ksize, stride, Hs, Ws, (a_rowmap ? 1 : 0) | (g_rowmap ? 2 : 0) | (g_scale ? 4 : 0));
    WgradArgs a{};
    a.x = (const uint16_t*)x; a.g = (const uint16_t*)grad_out; a.part = workspace; a.a_rowmap = a_rowmap; a.g_rowmap = g_rowmap;
    a.g_scale = g_scale; a.g_rows_per_sample = g_rows_per_sample > 0 ? g_rows_per_sample : 1;
    a.M = M; a.N = N; a.Cin = Cin; a.T = ksize * ksize; a.Hs = Hs; a.Ws = Ws; a.Ho = Ho; a.Wo = Wo; a.stride = stride; a.pad = ksize / 2;
    a.ctiles = r.ctiles; a.ntiles3 = r.ntiles3; a.nslices3 = r.nslices3; a.m_per_slice = r.m_per_slice;
    PK_REQUIRE(n_bias >= 0 && n_bias <= N && (!dbias || n_bias > 0), "pk_wgrad_bf16: n_bias");
    a.bias_part = n_bias > 0 ? workspace + (size_t)r.S * N * a.T * Cin : nullptr;     // bias slabs follow the weight slabs
    hipStream_t st = (hipStream_t)stream;
    PK_REQUIRE((int64_t)M * N < 0x3fffffffLL && (linear || (int64_t)B * Hs * Ws * Cin < 0x3fffffffLL), "pk_wgrad_bf16: tensor too large for 32-bit byte offsets");
    if (r.kernel == WG_WGRAD3) {
        PK_SUPPORTED(!linear && n_bias == 0, "pk_wgrad_bf16: the wide 3x3 kernel has no bias-gradient path (convolutions here carry no bias)");
    } else if (r.kernel != WG_WGRAD2) {
        if (r.kernel == WG_WGRAD4W && (a_rowmap || g_rowmap)) {
            const int nwin = ((Hs + 6) / 7) * ((Ws + 6) / 7);
            PK_REQUIRE(B > 0 && M == B * nwin * 49, "pk_wgrad_bf16: M = %d is not the window-order row count of a (%d, %d, %d) token grid", M, B, Hs, Ws);
            PK_REQUIRE(!g_scale || !g_rowmap || g_rows_per_sample == Hs * Ws, "pk_wgrad_bf16: g_rows_per_sample must be Hs * Ws with a window map");
            PK_REQUIRE((int64_t)B * Hs * Ws * (N > Cin ? N : Cin) < 0x3fffffffLL, "pk_wgrad_bf16: tensor too large for 32-bit byte offsets");
        }
        PK_SUPPORTED(r.kernel == WG_WGRAD4 || r.kernel == WG_WGRAD4W || n_bias == 0, "pk_wgrad_bf16: the 3x3 streaming kernel has no bias-gradient path (convolutions here carry no bias)");
        PK_REQUIRE(linear || r.kernel == WG_WGRAD4_COLS || (Ho == Hs && Wo == Ws), "pk_wgrad_bf16: stride-1 geometry");
        PK_REQUIRE((int64_t)r.rows * 2 < 0x3fffffffLL, "pk_wgrad_bf16: too many rows");
    }
    switch (wgrad_key(r.kernel, r.tn, r.tc, r.mode)) {
        WGRAD_CASE(WG_WGRAD2, 128, 128, 0, (k_wgrad2<128, 128, 32>))
        WGRAD_CASE(WG_WGRAD2, 64, 64, 0, (k_wgrad2<64, 64, 32>))
        case wgrad_key(WG_WGRAD3, 256, 256, 0): {
            static bool attr_set = false;
            const hipError_t e = attr_set ? hipSuccess : hipFuncSetAttribute((const void*)k_wgrad3, hipFuncAttributeMaxDynamicSharedMemorySize, r.lds);
            PK_REQUIRE(e == hipSuccess, "pk_wgrad_bf16: cannot reserve %d bytes of LDS: %s", r.lds, hipGetErrorString(e));
            attr_set = true;
            hipLaunchKernelGGL(k_wgrad3, r.grid, r.block, r.lds, st, a);
        } break;
        WGRAD_CASE(WG_WGRAD4, 64, 64, 0, (k_wgrad4<64, 64>))
        WGRAD_CASE(WG_WGRAD4, 64, 128, 0, (k_wgrad4<64, 128>))
        WGRAD_CASE(WG_WGRAD4, 128, 64, 0, (k_wgrad4<128, 64>))
        WGRAD_CASE(WG_WGRAD4, 128, 128, 0, (k_wgrad4<128, 128>))
        WGRAD_CASE(WG_WGRAD4_COLS, 64, 128, 0, (k_wgrad4<64, 128, true>))
        WGRAD_CASE(WG_WGRAD4_COLS, 128, 128, 0, (k_wgrad4<128, 128, true>))
        WGRAD_CASE(WG_WGRAD4_3X3, 64, 64, 0, k_wgrad4_3x3)
        WGRAD4W_CASES(64, 64) WGRAD4W_CASES(64, 128) WGRAD4W_CASES(128, 64) WGRAD4W_CASES(128, 128)
        default: pk_set_error("pk_wgrad_bf16: no kernel instantiation for route %d, tile %d x %d, mode %d", (int)r.kernel, r.tn, r.tc, r.mode); return PK_ERR_UNSUPPORTED;
    }
    if (!dw) return pk_launch_status("pk_wgrad_bf16");        // slabs only: the caller reduces them later (pk_reduce_many)
    const int total = N * a.T * Cin;
    const int w_blocks = (total + 15) / 16, b_blocks = dbias ? (n_bias + 15) / 16 : 0;
    hipLaunchKernelGGL(k_wgrad_reduce, dim3(w_blocks + b_blocks), dim3(256), 0, st, workspace, dw, r.S, N, a.T, Cin, out_layout,
                       a.bias_part, dbias, n_bias, w_blocks);
    return pk_launch_status("pk_wgrad_bf16");
}
