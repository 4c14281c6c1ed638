// BatchNorm: statistics finalize, apply (+ residual, ReLU), the fused small-tensor forms, backward; single problems and groups of layers.
#include "pk_rowops.h"

// ================================================================================================ BatchNorm (train)
// Finalize the per-tile column sums written by the conv epilogue: batch mean / biased var -> scale, shift for the
// apply kernel, saved mean / rstd for backward, running stats (momentum 0.1, UNBIASED var), num_batches_tracked += 1.
__global__ void __launch_bounds__(16 * RED_LANES) k_bn_finalize(const float* __restrict__ part, int tiles, int C, float count,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ run_mean, float* __restrict__ run_var,
                                                     long long* __restrict__ nbt, float momentum, float eps,
                                                     float* __restrict__ scale, float* __restrict__ shift,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out) {
    // block = 16 channels x 64 tile-lanes; fixed-order combination of the lane sums (deterministic)
    __shared__ double sh[2][RED_LANES][17];
    const int col = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + col;
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) nbt[0] += 1;
    double s = 0.0, q = 0.0;
    if (c < C) {
        int t = rl;
        for (; t + 3 * RED_LANES < tiles; t += 4 * RED_LANES) {       // eight independent loads per round
            const float* p0 = part + (size_t)t * 2 * C + c;
            const size_t st = (size_t)RED_LANES * 2 * C;
            const float s0 = p0[0], s1 = p0[st], s2 = p0[2 * st], s3 = p0[3 * st];
            const float q0 = p0[C], q1 = p0[st + C], q2 = p0[2 * st + C], q3 = p0[3 * st + C];
            s += ((double)s0 + (double)s1) + ((double)s2 + (double)s3);
            q += ((double)q0 + (double)q1) + ((double)q2 + (double)q3);
        }
        for (; t < tiles; t += RED_LANES) {
            s += (double)part[(size_t)t * 2 * C + c];
            q += (double)part[(size_t)t * 2 * C + C + c];
        }
    }
    sh[0][rl][col] = s;
    sh[1][rl][col] = q;
#pragma unroll
    for (int half = RED_LANES / 2; half >= 1; half >>= 1) {      // fixed binary tree (see k_sum_partials)
        __syncthreads();
        if (rl < half) {
            sh[0][rl][col] += sh[0][rl + half][col];
            sh[1][rl][col] += sh[1][rl + half][col];
        }
    }
    if (rl != 0 || c >= C) return;
    s = sh[0][0][col];
    q = sh[1][0][col];
    const double mean = s / count;
    double var = q / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float g = gamma[c];
    scale[c] = g * rstd;
    shift[c] = beta[c] - (float)mean * g * rstd;
    mean_out[c] = (float)mean;
    rstd_out[c] = rstd;
    if (run_mean) {
        const double unbiased = count > 1.f ? var * (double)count / ((double)count - 1.0) : var;
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unbiased;
    }
}
extern "C" int pk_bn_finalize(const float* stats_partial, int tiles, int C, int count, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                              float* scale, float* shift, float* save_mean, float* save_rstd, void* stream) {
    PK_REQUIRE(stats_partial && gamma && beta && scale && shift && save_mean && save_rstd, "pk_bn_finalize: null pointer");
    PK_REQUIRE(tiles > 0 && C > 0 && count > 0, "pk_bn_finalize: bad sizes");
    hipLaunchKernelGGL(k_bn_finalize, dim3((C + 15) / 16), dim3(16 * RED_LANES), 0, (hipStream_t)stream, stats_partial, tiles, C, (float)count,
                       gamma, beta, running_mean, running_var, (long long*)num_batches_tracked, momentum, eps, scale, shift, save_mean,
                       save_rstd);
    return pk_launch_status("pk_bn_finalize");
}

// y = act(x*scale[c] + shift[c] (+ residual)); one 16-byte chunk per thread-iteration
__global__ void __launch_bounds__(256) k_bn_act(const uint4* __restrict__ x, const float* __restrict__ scale,
                                                const float* __restrict__ shift, const uint4* __restrict__ res, uint4* __restrict__ y,
                                                size_t chunks, int cchunks, int relu, uint8_t* __restrict__ mask) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (size_t)gridDim.x * blockDim.x) {
        // (32-bit: a size_t modulo is a ~60-instruction software division per chunk; a mask when the chunk count is a power of two)
        const int c0 = (int)(((cchunks & (cchunks - 1)) == 0) ? ((uint32_t)i & (uint32_t)(cchunks - 1)) : ((uint32_t)i % (uint32_t)cchunks)) * 8;
        float v[8], r[8];
        unpack8(x[i], v);
        if (res) unpack8(res[i], r);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = v[j] * scale[c0 + j] + shift[c0 + j];
            if (res) t += r[j];
            v[j] = relu ? fmaxf(t, 0.f) : t;
        }
        const uint4 o = pack8(v);
        y[i] = o;
        if (mask) mask[i] = (uint8_t)pos_mask8(o);
    }
}
extern "C" int pk_bn_act(const void* x, const float* scale, const float* shift, const void* residual, void* y, int64_t rows, int C,
                         int relu, uint8_t* relu_mask, void* stream) {
    PK_REQUIRE(x && scale && shift && y && rows > 0 && C > 0 && (C & 7) == 0, "pk_bn_act: bad argument (C=%d)", C);
    const size_t chunks = (size_t)rows * (C / 8);
    unsigned nb;
    if (int rc = chunk_grid(chunks, 1, CHUNK_GRID_CAP, "pk_bn_act", nb)) return rc;
    hipLaunchKernelGGL(k_bn_act, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, scale, shift,
                       (const uint4*)residual, (uint4*)y, chunks, C / 8, relu, relu_mask);
    return pk_launch_status("pk_bn_act");
}

// Small tensors (<= BNS_MAX_TILES statistics rows, i.e. the low-resolution branches and their exchange units): finalize + apply in ONE
// launch.  Each workgroup owns 32 channels x a block of rows and first reduces the partial statistics of ITS 32 channels itself (8 row
// lanes per channel, fixed order, double: every workgroup computes bit-identical scale / shift), row block 0 also writes save_mean /
// save_rstd and the running statistics.  One launch (~7 us of fixed cost on a latency-bound chain) less per layer.
#define BNS_MAX_TILES 128
#define BNS_CG 32
__device__ __forceinline__ void bn_act_fin_body(const uint4* __restrict__ x, const float* __restrict__ part, int tiles, int C, float count,
                                                const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ run_mean,
                                                float* __restrict__ run_var, long long* __restrict__ nbt, float momentum, float eps,
                                                float* __restrict__ mean_out, float* __restrict__ rstd_out, const uint4* __restrict__ res,
                                                uint4* __restrict__ y, int rows, int rows_per_block, int relu, const int cg, const int rb,
                                                uint8_t* __restrict__ mask) {
    __shared__ double shs[8][BNS_CG], shq[8][BNS_CG];
    __shared__ float s_scale[BNS_CG], s_shift[BNS_CG];
    const int c0 = cg * BNS_CG;
    {
        const int cl = threadIdx.x & (BNS_CG - 1), pl = threadIdx.x >> 5, c = c0 + cl;
        double sm = 0.0, sq = 0.0;
        if (c < C)
            for (int t = pl; t < tiles; t += 8) {
                sm += (double)part[(size_t)t * 2 * C + c];
                sq += (double)part[(size_t)t * 2 * C + C + c];
            }
        shs[pl][cl] = sm;
        shq[pl][cl] = sq;
    }
    __syncthreads();
    if (threadIdx.x < BNS_CG && c0 + threadIdx.x < C) {
        const int cl = threadIdx.x, c = c0 + cl;
        double sm = 0.0, sq = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            sm += shs[k][cl];
            sq += shq[k][cl];
        }
        const double mean = sm / count;
        double var = sq / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        const float g = gamma[c];
        s_scale[cl] = g * rstd;
        s_shift[cl] = beta[c] - (float)mean * g * rstd;
        if (rb == 0) {
            mean_out[c] = (float)mean;
            rstd_out[c] = rstd;
            if (run_mean) {
                const double unbiased = count > 1.f ? var * (double)count / ((double)count - 1.0) : var;
                run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
                run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unbiased;
            }
            if (cg == 0 && cl == 0 && nbt) nbt[0] += 1;
        }
    }
    __syncthreads();
    const int cchunks = C / 8, ch = cg * (BNS_CG / 8) + (threadIdx.x & 3);
    if (ch >= cchunks) return;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = s_scale[(threadIdx.x & 3) * 8 + j];
        sh[j] = s_shift[(threadIdx.x & 3) * 8 + j];
    }
    const int r1 = min(rows, (rb + 1) * rows_per_block);
    for (int r = rb * rows_per_block + (threadIdx.x >> 2); r < r1; r += 64) {
        const size_t i = (size_t)r * cchunks + ch;
        float v[8], rr[8];
        unpack8(x[i], v);
        if (res) unpack8(res[i], rr);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = v[j] * sc[j] + sh[j];
            if (res) t += rr[j];
            v[j] = relu ? fmaxf(t, 0.f) : t;
        }
        const uint4 o = pack8(v);
        y[i] = o;
        if (mask) mask[i] = (uint8_t)pos_mask8(o);
    }
}
__global__ void __launch_bounds__(256) k_bn_act_fin(const uint4* __restrict__ x, const float* __restrict__ part, int tiles, int C, float count,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ run_mean,
                                                    float* __restrict__ run_var, long long* __restrict__ nbt, float momentum, float eps,
                                                    float* __restrict__ mean_out, float* __restrict__ rstd_out, const uint4* __restrict__ res,
                                                    uint4* __restrict__ y, int rows, int rows_per_block, int relu, uint8_t* __restrict__ mask) {
    bn_act_fin_body(x, part, tiles, C, count, gamma, beta, run_mean, run_var, nbt, momentum, eps, mean_out, rstd_out, res, y, rows, rows_per_block,
                    relu, (int)blockIdx.x, (int)blockIdx.y, mask);
}
// grouped form: up to PK_GROUP_MAX BatchNorm layers (any row count: every workgroup re-derives the statistics of its 32 channels)
struct BnFwdGroup {
    PkBnFwdDesc d[PK_GROUP_MAX];
    int first[PK_GROUP_MAX + 1], ncg[PK_GROUP_MAX], rpb[PK_GROUP_MAX];
    int n;
};
__global__ void __launch_bounds__(256) k_bn_act_fin_g(BnFwdGroup g) {
    const int L = (int)blockIdx.x;
    PK_GROUP_MEMBER(i, g.first, g.n, L);
    const PkBnFwdDesc& d = g.d[i];
    const int local = L - g.first[i], ncg = g.ncg[i];
    bn_act_fin_body((const uint4*)d.raw, d.stats_partial, d.tiles, d.C, (float)d.rows, d.gamma, d.beta, d.running_mean, d.running_var,
                    (long long*)d.num_batches_tracked, d.momentum, d.eps, d.save_mean, d.save_rstd, (const uint4*)d.residual, (uint4*)d.y,
                    (int)d.rows, g.rpb[i], d.relu, local % ncg, local / ncg, d.relu_mask);
}
// The workgroups of the fused kernels (k_bn_act_fin, k_bn_bwd_apply_fin and their grouped forms): ncg channel groups x nrb row blocks of
// rpb rows.  The single and the grouped entries of both directions take it from here.
struct BnFinGrid { int ncg, nrb, rpb; };
static inline BnFinGrid bn_fin_grid(int64_t rows, int C) {
    BnFinGrid g;
    g.ncg = (C + BNS_CG - 1) / BNS_CG;
    g.nrb = (int)((rows + 127) / 128);                       // >= 128 rows per workgroup, ~256 workgroups in all
    const int want = (256 + g.ncg - 1) / g.ncg;
    if (g.nrb > want) g.nrb = want;
    if (g.nrb < 1) g.nrb = 1;
    g.rpb = (int)((rows + g.nrb - 1) / g.nrb);
    return g;
}
extern "C" int pk_bn_train_fwd_group(const PkBnFwdDesc* d, int n, void* stream) {
    PK_REQUIRE(d && n > 0 && n <= PK_GROUP_MAX, "pk_bn_train_fwd_group: 1..%d members, got %d", PK_GROUP_MAX, n);
    BnFwdGroup g{};
    int total = 0;
    for (int i = 0; i < n; ++i) {
        const PkBnFwdDesc& c = d[i];
        PK_REQUIRE(c.raw && c.stats_partial && c.gamma && c.beta && c.y && c.save_mean && c.save_rstd, "pk_bn_train_fwd_group: null pointer");
        PK_REQUIRE(c.tiles > 0 && c.C > 0 && (c.C & 7) == 0 && c.rows > 0 && c.rows < (1 << 30), "pk_bn_train_fwd_group: bad sizes");
        g.d[i] = c;
        const BnFinGrid fg = bn_fin_grid(c.rows, c.C);
        g.ncg[i] = fg.ncg;
        g.rpb[i] = fg.rpb;
        g.first[i] = total;
        total += fg.ncg * fg.nrb;
    }
    g.first[n] = total;
    g.n = n;
    hipLaunchKernelGGL(k_bn_act_fin_g, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, g);
    return pk_launch_status("pk_bn_train_fwd_group");
}

// Train-mode BatchNorm forward from the conv epilogue's partial statistics: finalize + apply.  One fused launch for small tensors, the
// two kernels above otherwise.  `scale` / `shift`: [C] workspaces of the two-launch path.
extern "C" int pk_bn_train_fwd(const void* raw, const float* stats_partial, int tiles, int C, int64_t rows, const float* gamma,
                               const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                               float eps, const void* residual, void* y, float* save_mean, float* save_rstd, float* scale, float* shift,
                               int relu, uint8_t* relu_mask, void* stream) {
    PK_REQUIRE(raw && stats_partial && gamma && beta && y && save_mean && save_rstd && scale && shift, "pk_bn_train_fwd: null pointer");
    PK_REQUIRE(tiles > 0 && C > 0 && (C & 7) == 0 && rows > 0, "pk_bn_train_fwd: bad sizes");
    if (tiles <= BNS_MAX_TILES && rows <= 32768) {
        const BnFinGrid fg = bn_fin_grid(rows, C);
        hipLaunchKernelGGL(k_bn_act_fin, dim3(fg.ncg, fg.nrb), dim3(256), 0, (hipStream_t)stream, (const uint4*)raw, stats_partial, tiles, C, (float)rows,
                           gamma, beta, running_mean, running_var, (long long*)num_batches_tracked, momentum, eps, save_mean, save_rstd,
                           (const uint4*)residual, (uint4*)y, (int)rows, fg.rpb, relu, relu_mask);
        return pk_launch_status("pk_bn_train_fwd");
    }
    int rc = pk_bn_finalize(stats_partial, tiles, C, (int)rows, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, scale,
                            shift, save_mean, save_rstd, stream);
    if (rc) return rc;
    return pk_bn_act(raw, scale, shift, residual, y, rows, C, relu, relu_mask, stream);
}

// Backward, pass 1: per-block partial sums over rows of g and g*xhat, g = dy * (y > 0 if relu).
// (Measured and dropped: recomputing the ReLU mask from `raw` (scale/shift of the forward) to skip the read of `y` in both passes
// made the step SLOWER, 21.97 -> 25.4 ms even with the path disabled at run time: the extra per-channel state costs these
// bandwidth-bound kernels more than the saved 2 bytes per element.)
// Block = 256 threads = (256/cchunks) row lanes x cchunks channel chunks; partial[block][2][C].
// (The decode of the ReLU bits `mb` stays written out at its three sites: behind a __forceinline__ helper the compiler emits other code
// for k_bn_bwd_reduce, k_bn_bwd_reduce_g and k_bn_bwd_apply -- scripts/compare_kernels.py against the build before.)
#define BNR_MAXC 1024
__device__ __forceinline__ void bn_bwd_reduce_body(const uint4* __restrict__ dy, const uint4* __restrict__ yact,
                                                   const uint4* __restrict__ raw, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, float* __restrict__ part, int64_t rows, int C,
                                                   int relu, int rows_per_block, const int bid, const uint8_t* __restrict__ mask) {
    __shared__ float sh[256 * 16];
    const int cchunks = C / 8, rlanes = 256 / cchunks;
    const int cc = threadIdx.x % cchunks, rl = threadIdx.x / cchunks;
    float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float mu[8], rs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mu[j] = mean[cc * 8 + j];
        rs[j] = rstd[cc * 8 + j];
    }
    const int64_t r0 = (int64_t)bid * rows_per_block, r1 = min(rows, r0 + (int64_t)rows_per_block);
    if (rl < rlanes) {
        for (int64_t r = r0 + rl; r < r1; r += rlanes) {
            const size_t i = (size_t)r * cchunks + cc;
            float g[8], xr[8], ya[8];
            unpack8(dy[i], g);
            unpack8(raw[i], xr);
            uint32_t mb = 0xffu;
            if (relu) {
                if (mask) mb = mask[i];
                else {
                    unpack8(yact[i], ya);
                    mb = 0;
#pragma unroll
                    for (int j = 0; j < 8; ++j) mb |= (ya[j] > 0.f ? 1u : 0u) << j;
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float gg = ((mb >> j) & 1u) ? g[j] : 0.f;
                s1[j] += gg;
                s2[j] += gg * (xr[j] - mu[j]) * rs[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sh[threadIdx.x * 16 + j] = s1[j];
        sh[threadIdx.x * 16 + 8 + j] = s2[j];
    }
    __syncthreads();
    if (threadIdx.x < cchunks) {
        float a1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < rlanes; ++k) {
            const int t = k * cchunks + threadIdx.x;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a1[j] += sh[t * 16 + j];
                a2[j] += sh[t * 16 + 8 + j];
            }
        }
        float* dst = part + (size_t)bid * 2 * C;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            dst[threadIdx.x * 8 + j] = a1[j];
            dst[C + threadIdx.x * 8 + j] = a2[j];
        }
    }
}
__global__ void __launch_bounds__(256) k_bn_bwd_reduce(const uint4* __restrict__ dy, const uint4* __restrict__ yact,
                                                       const uint4* __restrict__ raw, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, float* __restrict__ part, int64_t rows, int C,
                                                       int relu, int rows_per_block, const uint8_t* __restrict__ mask) {
    bn_bwd_reduce_body(dy, yact, raw, mean, rstd, part, rows, C, relu, rows_per_block, (int)blockIdx.x, mask);
}
// Backward, pass 2: dx = gamma*rstd*(g - sum_g/M - xhat*sum_gx/M); optional d_residual = g
__global__ void __launch_bounds__(256) k_bn_bwd_apply(const uint4* __restrict__ dy, const uint4* __restrict__ yact,
                                                      const uint4* __restrict__ raw, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                      const float* __restrict__ sums, float inv_count, uint4* __restrict__ dx,
                                                      uint4* __restrict__ dres, size_t chunks, int cchunks, int relu,
                                                      const uint8_t* __restrict__ mask) {
    const int C = cchunks * 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (size_t)gridDim.x * blockDim.x) {
        // (32-bit: a size_t modulo is a ~60-instruction software division per chunk; a mask when the chunk count is a power of two)
        const int c0 = (int)(((cchunks & (cchunks - 1)) == 0) ? ((uint32_t)i & (uint32_t)(cchunks - 1)) : ((uint32_t)i % (uint32_t)cchunks)) * 8;
        float g[8], xr[8], ya[8], o[8];
        unpack8(dy[i], g);
        unpack8(raw[i], xr);
        uint32_t mb = 0xffu;
        if (relu) {
            if (mask) mb = mask[i];
            else {
                unpack8(yact[i], ya);
                mb = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) mb |= (ya[j] > 0.f ? 1u : 0u) << j;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j;
            const float gg = ((mb >> j) & 1u) ? g[j] : 0.f;
            g[j] = gg;
            const float xh = (xr[j] - mean[c]) * rstd[c];
            o[j] = gamma[c] * rstd[c] * (gg - sums[c] * inv_count - xh * sums[C + c] * inv_count);
        }
        dx[i] = pack8(o);
        if (dres) dres[i] = pack8(g);
    }
}
// (max_rows / small_nb, measured on HRNet-W32 384x288 training, 22.23 ms per step at the defaults: 262 144 rows with 128 / 256
// partial rows 23.57 / 23.06 ms, 65 536 rows with 128 partial rows 22.29 ms -- the large tensors keep the three-launch form)
static inline bool bn_bwd_small(int64_t rows) {
    constexpr long max_rows = 32768;
    return rows <= max_rows;
}
extern "C" int pk_bn_bwd_blocks(int64_t rows) {
    // >= 32 rows per block, up to 1024 blocks: the low-resolution branches (3 072 .. 12 288 rows) still get hundreds of
    // workgroups (rows/256 left them with 12 .. 48 and a 55 us kernel for 3 MB of data).  Small tensors: at most 64 blocks, because
    // every workgroup of the fused apply kernel re-reduces the partial sums of its 32 channels itself (64 x 2 x 32 floats = 16 KB).
    int64_t nb = (rows + 31) / 32;
    constexpr int small_nb = 64;
    if (bn_bwd_small(rows) && nb > small_nb) nb = small_nb;
    return (int)(nb > 1024 ? 1024 : (nb < 1 ? 1 : nb));
}
// Small tensors: pass 2 with the partial-sum reduction folded in (see k_bn_act_fin): each workgroup owns 32 channels x a block of rows,
// reduces partial[nb][2][C] for its channels (8 lanes, fixed order, double), row block 0 writes dbeta / dgamma; then dx (and dres).
__device__ __forceinline__ void bn_bwd_apply_fin_body(const uint4* __restrict__ dy, const uint4* __restrict__ yact, const uint4* __restrict__ raw,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma, const float* __restrict__ part, int nb,
                                                      float inv_count, float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                      uint4* __restrict__ dx, uint4* __restrict__ dres, int rows, int rows_per_block, int C,
                                                      int relu, const int cg, const int rb, const uint8_t* __restrict__ mask) {
    __shared__ double sh1[8][BNS_CG], sh2[8][BNS_CG];
    __shared__ float s_1[BNS_CG], s_2[BNS_CG];
    const int c0 = cg * BNS_CG;
    {
        const int cl = threadIdx.x & (BNS_CG - 1), pl = threadIdx.x >> 5, c = c0 + cl;
        double a = 0.0, b = 0.0;
        if (c < C)
            for (int t = pl; t < nb; t += 8) {
                a += (double)part[(size_t)t * 2 * C + c];
                b += (double)part[(size_t)t * 2 * C + C + c];
            }
        sh1[pl][cl] = a;
        sh2[pl][cl] = b;
    }
    __syncthreads();
    if (threadIdx.x < BNS_CG && c0 + threadIdx.x < C) {
        const int cl = threadIdx.x;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a += sh1[k][cl];
            b += sh2[k][cl];
        }
        s_1[cl] = (float)a;
        s_2[cl] = (float)b;
        if (rb == 0) {
            dbeta[c0 + cl] = (float)a;
            dgamma[c0 + cl] = (float)b;
        }
    }
    __syncthreads();
    const int cchunks = C / 8, ch = cg * (BNS_CG / 8) + (threadIdx.x & 3);
    if (ch >= cchunks) return;
    float mu[8], rs[8], gm[8], t1[8], t2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = ch * 8 + j;
        mu[j] = mean[c];
        rs[j] = rstd[c];
        gm[j] = gamma[c] * rs[j];
        t1[j] = s_1[(threadIdx.x & 3) * 8 + j] * inv_count;
        t2[j] = s_2[(threadIdx.x & 3) * 8 + j] * inv_count;
    }
    const int r1 = min(rows, (rb + 1) * rows_per_block);
    for (int r = rb * rows_per_block + (threadIdx.x >> 2); r < r1; r += 64) {
        const size_t i = (size_t)r * cchunks + ch;
        float g[8], xr[8], ya[8], o[8];
        unpack8(dy[i], g);
        unpack8(raw[i], xr);
        uint32_t mb = 0xffu;
        if (relu) {
            if (mask) mb = mask[i];
            else {
                unpack8(yact[i], ya);
                mb = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) mb |= (ya[j] > 0.f ? 1u : 0u) << j;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float gg = ((mb >> j) & 1u) ? g[j] : 0.f;
            g[j] = gg;
            const float xh = (xr[j] - mu[j]) * rs[j];
            o[j] = gm[j] * (gg - t1[j] - xh * t2[j]);
        }
        dx[i] = pack8(o);
        if (dres) dres[i] = pack8(g);
    }
}
__global__ void __launch_bounds__(256) k_bn_bwd_apply_fin(const uint4* __restrict__ dy, const uint4* __restrict__ yact, const uint4* __restrict__ raw,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ part, int nb,
                                                          float inv_count, float* __restrict__ dbeta, float* __restrict__ dgamma,
                                                          uint4* __restrict__ dx, uint4* __restrict__ dres, int rows, int rows_per_block, int C,
                                                          int relu, const uint8_t* __restrict__ mask) {
    bn_bwd_apply_fin_body(dy, yact, raw, mean, rstd, gamma, part, nb, inv_count, dbeta, dgamma, dx, dres, rows, rows_per_block, C, relu,
                          (int)blockIdx.x, (int)blockIdx.y, mask);
}
// grouped backward: ONE reduce launch + ONE apply launch for up to PK_GROUP_MAX BatchNorm layers
struct BnBwdGroup {
    PkBnBwdDesc d[PK_GROUP_MAX];
    int first_r[PK_GROUP_MAX + 1], first_a[PK_GROUP_MAX + 1];
    int nb[PK_GROUP_MAX], rpb_r[PK_GROUP_MAX], ncg[PK_GROUP_MAX], rpb_a[PK_GROUP_MAX];
    int n;
};
__global__ void __launch_bounds__(256) k_bn_bwd_reduce_g(BnBwdGroup g) {
    const int L = (int)blockIdx.x;
    PK_GROUP_MEMBER(i, g.first_r, g.n, L);
    const PkBnBwdDesc& d = g.d[i];
    bn_bwd_reduce_body((const uint4*)d.dy, (const uint4*)d.y_act, (const uint4*)d.raw, d.save_mean, d.save_rstd, d.partial, d.rows, d.C, d.relu & 1,
                       g.rpb_r[i], L - g.first_r[i], d.relu_mask);
}
__global__ void __launch_bounds__(256) k_bn_bwd_apply_fin_g(BnBwdGroup g) {
    const int L = (int)blockIdx.x;
    PK_GROUP_MEMBER(i, g.first_a, g.n, L);
    const PkBnBwdDesc& d = g.d[i];
    const int local = L - g.first_a[i], ncg = g.ncg[i];
    bn_bwd_apply_fin_body((const uint4*)d.dy, (const uint4*)d.y_act, (const uint4*)d.raw, d.save_mean, d.save_rstd, d.gamma, d.partial, g.nb[i],
                          (d.relu & 2) ? 0.f : 1.f / (float)d.rows, d.dbeta, d.dgamma, (uint4*)d.dx, (uint4*)d.dresidual, (int)d.rows, g.rpb_a[i],
                          d.C, d.relu & 1, local % ncg, local / ncg, d.relu_mask);
}
// partial rows [blocks][2][C] of a member of pk_bn_bwd_group: the small-tensor rule of pk_bn_bwd where it applies (same sums bit for bit)
extern "C" int pk_bn_bwd_group_blocks(int64_t rows) {
    if (bn_bwd_small(rows)) return pk_bn_bwd_blocks(rows);
    const int64_t nb = (rows + 127) / 128;
    return (int)(nb > 256 ? 256 : nb);
}
// The reduce pass (k_bn_bwd_reduce, k_bn_bwd_reduce_g): nb workgroups of rpb consecutive rows, one partial row [2][C] each
struct BnReduceGrid { int nb, rpb; };
static inline BnReduceGrid bn_reduce_grid(int64_t rows, bool grouped) {
    BnReduceGrid g;
    g.nb = grouped ? pk_bn_bwd_group_blocks(rows) : pk_bn_bwd_blocks(rows);
    g.rpb = (int)((rows + g.nb - 1) / g.nb);
    return g;
}
extern "C" int pk_bn_bwd_group(const PkBnBwdDesc* d, int n, void* stream) {
    PK_REQUIRE(d && n > 0 && n <= PK_GROUP_MAX, "pk_bn_bwd_group: 1..%d members, got %d", PK_GROUP_MAX, n);
    BnBwdGroup g{};
    int tr = 0, ta = 0;
    for (int i = 0; i < n; ++i) {
        const PkBnBwdDesc& c = d[i];
        PK_REQUIRE(c.dy && c.raw && c.save_mean && c.save_rstd && c.gamma && c.partial && c.dgamma && c.dbeta && c.dx, "pk_bn_bwd_group: null pointer");
        PK_REQUIRE(!(c.relu & 1) || c.y_act || c.relu_mask, "pk_bn_bwd_group: relu needs the activated output or its bit mask");
        PK_REQUIRE(c.rows > 0 && c.rows < (1 << 30) && c.C > 0 && (c.C & 7) == 0, "pk_bn_bwd_group: bad sizes");
        PK_SUPPORTED(c.C <= BNR_MAXC && c.C / 8 <= 256, "pk_bn_bwd_group: C=%d too large", c.C);
        g.d[i] = c;
        const BnReduceGrid rg = bn_reduce_grid(c.rows, true);
        const BnFinGrid fg = bn_fin_grid(c.rows, c.C);
        g.nb[i] = rg.nb;
        g.rpb_r[i] = rg.rpb;
        g.ncg[i] = fg.ncg;
        g.rpb_a[i] = fg.rpb;
        g.first_r[i] = tr;
        g.first_a[i] = ta;
        tr += rg.nb;
        ta += fg.ncg * fg.nrb;
    }
    g.first_r[n] = tr;
    g.first_a[n] = ta;
    g.n = n;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bn_bwd_reduce_g, dim3((unsigned)tr), dim3(256), 0, st, g);
    hipLaunchKernelGGL(k_bn_bwd_apply_fin_g, dim3((unsigned)ta), dim3(256), 0, st, g);
    return pk_launch_status("pk_bn_bwd_group");
}

extern "C" int pk_bn_bwd(const void* dy, const void* y_act, const void* raw, const float* save_mean, const float* save_rstd,
                         const float* gamma, float* partial, float* sums, float* dgamma, float* dbeta, void* dx, void* dresidual,
                         int64_t rows, int C, int relu, const uint8_t* relu_mask, void* stream) {
    PK_REQUIRE(dy && raw && save_mean && save_rstd && gamma && partial && sums && dgamma && dbeta && dx, "pk_bn_bwd: null pointer");
    // relu: bit 0 = the forward applied ReLU; bit 1 = eval-mode BatchNorm (running statistics are constants: no batch-mean terms)
    const int eval_mode = relu & 2;
    relu &= 1;
    PK_REQUIRE(!relu || y_act || relu_mask, "pk_bn_bwd: relu needs the activated output or its bit mask");
    PK_REQUIRE(rows > 0 && C > 0 && (C & 7) == 0, "pk_bn_bwd: bad sizes");
    PK_SUPPORTED(C <= BNR_MAXC && C / 8 <= 256, "pk_bn_bwd: C=%d too large", C);
    const size_t chunks = (size_t)rows * (C / 8);
    unsigned gb;
    if (int rc = chunk_grid(chunks, 1, CHUNK_GRID_CAP, "pk_bn_bwd", gb)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const BnReduceGrid rg = bn_reduce_grid(rows, false);
    const int nb = rg.nb;
    hipLaunchKernelGGL(k_bn_bwd_reduce, dim3(nb), dim3(256), 0, st, (const uint4*)dy, (const uint4*)y_act, (const uint4*)raw, save_mean,
                       save_rstd, partial, rows, C, relu, rg.rpb, relu_mask);
    if (bn_bwd_small(rows)) {          // the reduction of the partial sums rides in the apply launch
        const BnFinGrid fg = bn_fin_grid(rows, C);
        hipLaunchKernelGGL(k_bn_bwd_apply_fin, dim3(fg.ncg, fg.nrb), dim3(256), 0, st, (const uint4*)dy, (const uint4*)y_act, (const uint4*)raw, save_mean,
                           save_rstd, gamma, partial, nb, eval_mode ? 0.f : 1.f / (float)rows, dbeta, dgamma, (uint4*)dx, (uint4*)dresidual, (int)rows,
                           fg.rpb, C, relu, relu_mask);
        return pk_launch_status("pk_bn_bwd");
    }
    // sums = [sum g | sum g*xhat] for the apply kernel; the same values go to dbeta / dgamma (possibly flat-gradient views)
    sum_partials_launch(partial, nb, 2 * C, 2 * C, sums, 1.f, 0, dbeta, dgamma, C, st);
    hipLaunchKernelGGL(k_bn_bwd_apply, dim3(gb), dim3(256), 0, st, (const uint4*)dy, (const uint4*)y_act, (const uint4*)raw,
                       save_mean, save_rstd, gamma, sums, eval_mode ? 0.f : 1.f / (float)rows, (uint4*)dx, (uint4*)dresidual, chunks, C / 8, relu, relu_mask);
    return pk_launch_status("pk_bn_bwd");
}

// relu backward alone (exchange-unit output / plain masks): dx = dy * (y > 0)
__global__ void __launch_bounds__(256) k_relu_bwd(const uint4* __restrict__ dy, const uint4* __restrict__ y, uint4* __restrict__ dx,
                                                  size_t chunks) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (size_t)gridDim.x * blockDim.x) {
        float g[8], v[8];
        unpack8(dy[i], g);
        unpack8(y[i], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = v[j] > 0.f ? g[j] : 0.f;
        dx[i] = pack8(g);
    }
}
extern "C" int pk_relu_bwd(const void* dy, const void* y, void* dx, int64_t numel, void* stream) {
    PK_REQUIRE(dy && y && dx && numel > 0 && (numel & 7) == 0, "pk_relu_bwd: bad argument");
    const size_t chunks = (size_t)numel / 8;
    unsigned gb;
    chunk_grid(chunks, 1, CHUNK_GRID_CAP, nullptr, gb);          // 64-bit chunk indices in the kernel: nothing to refuse
    hipLaunchKernelGGL(k_relu_bwd, dim3(gb), dim3(256), 0, (hipStream_t)stream, (const uint4*)dy, (const uint4*)y, (uint4*)dx, chunks);
    return pk_launch_status("pk_relu_bwd");
}
