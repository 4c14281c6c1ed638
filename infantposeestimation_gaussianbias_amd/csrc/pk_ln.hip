// LayerNorm (forward / backward), column sums of bf16 matrices, and the generic partial-sum reduction they and BatchNorm backward end in.
#include "pk_rowops.h"

// ================================================================================================ generic partial sums
// out[k] (+)= scale * sum_b partial[b*stride + k], k < K.  Block = 16 columns x 64 row-lanes: lane r sums rows b = r (mod 64),
// the 64 lane sums are combined in fixed order -> deterministic, and the serial chain is nb/64 instead of nb (these kernels
// sit between two passes of BatchNorm backward, i.e. on the critical path, with only K/16 workgroups).
__global__ void __launch_bounds__(16 * RED_LANES) k_sum_partials(const float* __restrict__ part, int nb, int K, int stride, float* __restrict__ out,
                                                      float scale, int accumulate, float* __restrict__ out_lo, float* __restrict__ out_hi,
                                                      int split) {
    __shared__ double sh[RED_LANES][17];
    const int col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int k = blockIdx.x * 16 + col;
    double s = 0.0;
    if (k < K) {
        // four independent loads per round: the serial chain is memory latency x nb / 256, not x nb / 64
        int b = rl;
        for (; b + 3 * RED_LANES < nb; b += 4 * RED_LANES) {
            const float v0 = part[(size_t)b * stride + k], v1 = part[(size_t)(b + RED_LANES) * stride + k];
            const float v2 = part[(size_t)(b + 2 * RED_LANES) * stride + k], v3 = part[(size_t)(b + 3 * RED_LANES) * stride + k];
            s += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
        }
        for (; b < nb; b += RED_LANES) s += (double)part[(size_t)b * stride + k];
    }
    sh[rl][col] = s;
    // fixed binary tree over the 64 lane sums (a single thread adding them one after the other was 64 dependent LDS round trips:
    // ~2.5 us of a 7 us kernel that sits between two passes of BatchNorm backward)
#pragma unroll
    for (int half = RED_LANES / 2; half >= 1; half >>= 1) {
        __syncthreads();
        if (rl < half) sh[rl][col] += sh[rl + half][col];
    }
    if (rl == 0 && k < K) {
        const double t = sh[0][col];
        const float v = (float)t * scale;
        if (out) out[k] = accumulate ? out[k] + v : v;
        if (out_lo && k < split) out_lo[k] = v;            // optional second copy, split into two destinations
        if (out_hi && k >= split) out_hi[k - split] = v;
    }
}
void sum_partials_launch(const float* partial, int nb, int K, int stride, float* out, float scale, int accumulate, float* out_lo, float* out_hi, int split,
                         hipStream_t stream) {
    hipLaunchKernelGGL(k_sum_partials, dim3((K + 15) / 16), dim3(16 * RED_LANES), 0, stream, partial, nb, K, stride, out, scale, accumulate, out_lo, out_hi,
                       split);
}
extern "C" int pk_sum_partials(const float* partial, int nb, int K, int stride, float* out, float scale, int accumulate, void* stream) {
    PK_REQUIRE(partial && out && nb > 0 && K > 0 && stride >= K, "pk_sum_partials: bad argument");
    sum_partials_launch(partial, nb, K, stride, out, scale, accumulate, nullptr, nullptr, 0, (hipStream_t)stream);
    return pk_launch_status("pk_sum_partials");
}

// ================================================================================================ LayerNorm
// Row of C channels handled by L = pow2 >= C/(8*CPL) lanes, CPL chunks of 8 channels per lane (CPL = 2 only for C > 512);
// 64/L rows per wave.  `Cr` (<= C) is the number of REAL channels: statistics are taken over the first Cr channels only
// (the padded twin of HRFormer-base keeps 78 real channels in 80-wide rows; padded inputs are zero, padded outputs are
// forced to zero) -- Cr == C for every natively supported model.
template <int L, int CPL>
__global__ void __launch_bounds__(256) k_ln_fwd(const uint4* __restrict__ x, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, uint4* __restrict__ y, float* __restrict__ mean_out,
                                                float* __restrict__ rstd_out, int64_t rows, int C, int Cr, float eps) {
    const int cchunks = C / 8, sub = threadIdx.x % L;
    const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / L;
    float v[CPL][8];
    bool on[CPL];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int ch = sub + c * L;
        on[c] = row < rows && ch < cchunks;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[c][j] = 0.f;
        if (on[c]) unpack8(x[(size_t)row * cchunks + ch], v[c]);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += (ch * 8 + j < Cr) ? v[c][j] : 0.f;
    }
    s = lanes_sum<L>(s);
    const float mean = s / (float)Cr;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int ch = sub + c * L;
        if (on[c]) {
#pragma unroll
            for (int j = 0; j < 8; ++j) q += (ch * 8 + j < Cr) ? (v[c][j] - mean) * (v[c][j] - mean) : 0.f;
        }
    }
    q = lanes_sum<L>(q);
    const float rstd = rsqrtf(q / (float)Cr + eps);
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int ch = sub + c * L;
        if (!on[c]) continue;
        // gamma / beta have C entries (the padded ones are ignored): unconditional 16-byte loads, select afterwards
        const float4 g0 = *reinterpret_cast<const float4*>(gamma + ch * 8), g1 = *reinterpret_cast<const float4*>(gamma + ch * 8 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(beta + ch * 8), b1 = *reinterpret_cast<const float4*>(beta + ch * 8 + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float t = (v[c][j] - mean) * rstd * gg[j] + bb[j];
            v[c][j] = (ch * 8 + j < Cr) ? t : 0.f;
        }
        y[(size_t)row * cchunks + ch] = pack8(v[c]);
    }
    if (sub == 0 && row < rows) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
    }
}
static int ln_lanes(int C) {
    int l = 1;
    while (l * 8 < C && l < 64) l <<= 1;
    return l;
}
// One launch of KERNEL<L, CPL> for rows of C channels; GRID(L): the workgroup count for L lanes per row
#define LN_LAUNCH(KERNEL, L, CPL, GRID, ...) hipLaunchKernelGGL((KERNEL<L, CPL>), dim3((unsigned)GRID(L)), dim3(256), 0, st, __VA_ARGS__)
#define LN_DISPATCH(KERNEL, GRID, ...)                                      \
    do {                                                                    \
        if (C > 512) LN_LAUNCH(KERNEL, 64, 2, GRID, __VA_ARGS__);           \
        else switch (ln_lanes(C)) {                                         \
            case 1: LN_LAUNCH(KERNEL, 1, 1, GRID, __VA_ARGS__); break;      \
            case 2: LN_LAUNCH(KERNEL, 2, 1, GRID, __VA_ARGS__); break;      \
            case 4: LN_LAUNCH(KERNEL, 4, 1, GRID, __VA_ARGS__); break;      \
            case 8: LN_LAUNCH(KERNEL, 8, 1, GRID, __VA_ARGS__); break;      \
            case 16: LN_LAUNCH(KERNEL, 16, 1, GRID, __VA_ARGS__); break;    \
            case 32: LN_LAUNCH(KERNEL, 32, 1, GRID, __VA_ARGS__); break;    \
            default: LN_LAUNCH(KERNEL, 64, 1, GRID, __VA_ARGS__); break;    \
        }                                                                   \
    } while (0)
extern "C" int pk_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* save_mean, float* save_rstd,
                                int64_t rows, int C, int C_real, float eps, void* stream) {
    PK_REQUIRE(x && gamma && beta && y && save_mean && save_rstd && rows > 0, "pk_layernorm_fwd: bad argument");
    PK_SUPPORTED(C >= 8 && (C & 7) == 0 && C <= 1024, "pk_layernorm_fwd: C=%d (need a multiple of 8, <= 1024)", C);
    const int Cr = C_real > 0 ? C_real : C;
    PK_REQUIRE(Cr <= C, "pk_layernorm_fwd: C_real=%d > C=%d", Cr, C);
    hipStream_t st = (hipStream_t)stream;
    const auto grid = [&](int lanes) { return (rows * lanes + 255) / 256; };
    LN_DISPATCH(k_ln_fwd, grid, (const uint4*)x, gamma, beta, (uint4*)y, save_mean, save_rstd, rows, C, Cr, eps);
    return pk_launch_status("pk_layernorm_fwd");
}

// dx = rstd*(gh - mean_c(gh) - xhat*mean_c(gh*xhat)) (+ dres), gh = dy*gamma; per-block partials of dgamma/dbeta.
// Each block owns `rows_per_block` consecutive rows so its column partials can be reduced deterministically.
template <int L, int CPL>
__global__ void __launch_bounds__(256) k_ln_bwd(const uint4* __restrict__ dy, const uint4* __restrict__ x, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                const uint4* __restrict__ dres, uint4* __restrict__ dx, float* __restrict__ part,
                                                int64_t rows, int C, int Cr, int rows_per_block) {
    __shared__ float sh[256 * 16];
    const int cchunks = C / 8, sub = threadIdx.x % L, rl = threadIdx.x / L, rlanes = 256 / L;
    float* dst = part + (size_t)blockIdx.x * 2 * C;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + (int64_t)rows_per_block);
    float ag[CPL][8], ab[CPL][8], gm[CPL][8];
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = (sub + c * L) * 8 + j;
            ag[c][j] = ab[c][j] = 0.f;
            gm[c][j] = (col < C) ? gamma[col] : 0.f;      // C entries; padded columns are masked where they are used
            if (col >= Cr) gm[c][j] = 0.f;
        }
    for (int64_t rb = r0; rb < r1; rb += rlanes) {        // uniform trip count: every lane executes the shuffles
        const int64_t row = rb + rl;
        float g[CPL][8], xh[CPL][8];
        float mu = 0.f, rs = 0.f;
        if (row < r1) {
            mu = mean[row];
            rs = rstd[row];
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int ch = sub + c * L;
            const bool on = row < r1 && ch < cchunks;
            float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) g[c][j] = 0.f;
            if (on) {
                unpack8(dy[(size_t)row * cchunks + ch], g[c]);
                unpack8(x[(size_t)row * cchunks + ch], v);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool real = ch * 8 + j < Cr;
                xh[c][j] = real ? (v[j] - mu) * rs : 0.f;
                if (!real) g[c][j] = 0.f;
                const float gh = g[c][j] * gm[c][j];
                s1 += gh;
                s2 += gh * xh[c][j];
                ag[c][j] += g[c][j] * xh[c][j];
                ab[c][j] += g[c][j];
            }
        }
        s1 = lanes_sum<L>(s1);
        s2 = lanes_sum<L>(s2);
        const float m1 = s1 / (float)Cr, m2 = s2 / (float)Cr;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int ch = sub + c * L;
            if (!(row < r1 && ch < cchunks)) continue;
            float o8[8], r8[8];
            if (dres) unpack8(dres[(size_t)row * cchunks + ch], r8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                o8[j] = (ch * 8 + j < Cr) ? rs * (g[c][j] * gm[c][j] - m1 - xh[c][j] * m2) : 0.f;
                if (dres) o8[j] += r8[j];
            }
            dx[(size_t)row * cchunks + ch] = pack8(o8);
        }
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sh[threadIdx.x * 16 + j] = ag[c][j];
            sh[threadIdx.x * 16 + 8 + j] = ab[c][j];
        }
        __syncthreads();
        const int ch = threadIdx.x + c * L;
        if (threadIdx.x < L && ch < cchunks) {
            float a1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < rlanes; ++k) {
                const int t = k * L + threadIdx.x;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    a1[j] += sh[t * 16 + j];
                    a2[j] += sh[t * 16 + 8 + j];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                dst[ch * 8 + j] = a1[j];
                dst[C + ch * 8 + j] = a2[j];
            }
        }
    }
}
extern "C" int pk_ln_bwd_blocks(int64_t rows) {
    int64_t nb = (rows + 31) / 32;             // see pk_bn_bwd_blocks
    return (int)(nb > 1024 ? 1024 : (nb < 1 ? 1 : nb));
}
extern "C" int pk_layernorm_bwd(const void* dy, const void* x, const float* save_mean, const float* save_rstd, const float* gamma,
                                const void* dresidual, void* dx, float* partial, float* dgamma, float* dbeta, int64_t rows, int C,
                                int C_real, void* stream) {
    PK_REQUIRE(dy && x && save_mean && save_rstd && gamma && dx && partial && rows > 0 && (!dgamma == !dbeta), "pk_layernorm_bwd: bad argument");
    PK_SUPPORTED(C >= 8 && (C & 7) == 0 && C <= 1024, "pk_layernorm_bwd: C=%d", C);
    const int Cr = C_real > 0 ? C_real : C;
    PK_REQUIRE(Cr <= C, "pk_layernorm_bwd: C_real=%d > C=%d", Cr, C);
    hipStream_t st = (hipStream_t)stream;
    const int nb = pk_ln_bwd_blocks(rows);
    const int rpb = (int)((rows + nb - 1) / nb);
    const auto grid = [&](int) { return nb; };
    LN_DISPATCH(k_ln_bwd, grid, (const uint4*)dy, (const uint4*)x, save_mean, save_rstd, gamma, (const uint4*)dresidual, (uint4*)dx, partial, rows, C, Cr, rpb);
    if (!dgamma) return pk_launch_status("pk_layernorm_bwd");   // partials only: reduced later by pk_reduce_many
    sum_partials_launch(partial, nb, 2 * C, 2 * C, nullptr, 1.f, 0, dgamma, dbeta, C, st);
    return pk_launch_status("pk_layernorm_bwd");
}

// column sums of a bf16 [rows][N] matrix (bias gradients): partial[block][N] then k_sum_partials
__global__ void __launch_bounds__(256) k_colsum(const uint4* __restrict__ g, const int32_t* __restrict__ rowmap, float* __restrict__ part,
                                                int64_t rows, int N, int rows_per_block, const float* __restrict__ row_scale,
                                                int rows_per_sample) {
    __shared__ float sh[256 * 8];
    const int cchunks = N / 8, rlanes = 256 / cchunks;
    const int cc = threadIdx.x % cchunks, rl = threadIdx.x / cchunks;
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + (int64_t)rows_per_block);
    if (rl < rlanes)
        for (int64_t r = r0 + rl; r < r1; r += rlanes) {
            const int64_t src = rowmap ? rowmap[r] : r;
            if (src < 0) continue;
            float v[8];
            unpack8(g[(size_t)src * cchunks + cc], v);
            const float sc = row_scale ? row_scale[src / rows_per_sample] : 1.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] += v[j] * sc;
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[threadIdx.x * 8 + j] = a[j];
    __syncthreads();
    if (threadIdx.x < cchunks) {
        float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < rlanes; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += sh[(k * cchunks + threadIdx.x) * 8 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) part[(size_t)blockIdx.x * N + threadIdx.x * 8 + j] = s[j];
    }
}
extern "C" int pk_colsum_bf16(const void* g, const int32_t* rowmap, const float* row_scale, int rows_per_sample, float* partial,
                              float* out, int64_t rows, int N, void* stream) {
    PK_REQUIRE(g && partial && out && rows > 0 && N > 0 && (N & 7) == 0, "pk_colsum_bf16: bad argument");
    PK_REQUIRE(!row_scale || rows_per_sample > 0, "pk_colsum_bf16: row_scale needs rows_per_sample");
    PK_SUPPORTED(N / 8 <= 256, "pk_colsum_bf16: N=%d too wide", N);
    const int nb = pk_ln_bwd_blocks(rows);
    const int rpb = (int)((rows + nb - 1) / nb);
    hipLaunchKernelGGL(k_colsum, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const uint4*)g, rowmap, partial, rows, N, rpb, row_scale,
                       rows_per_sample > 0 ? rows_per_sample : 1);
    sum_partials_launch(partial, nb, N, N, out, 1.f, 0, nullptr, nullptr, 0, (hipStream_t)stream);
    return pk_launch_status("pk_colsum_bf16");
}
