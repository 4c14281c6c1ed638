// Heatmap decoders (D1-D4): everything that turns heatmaps into coordinates or merges heatmaps.  HBM-bound, fp32.
#include "pk_common.h"

// ================================================================================================ argmax (D2, D3)
// One workgroup per map with 32-bit indices inside it: what the entries that take an argmax over a map, or gather from one, ask of a shape
static inline bool map_shape_ok(int maps, int H, int W) { return maps > 0 && H > 0 && W > 0 && (int64_t)H * W < 0x7fffffff; }
struct ArgMax {
    float v;
    int i;
};
// torch.max semantics: NaN counts as the maximum; ties resolve to the lowest flat index.
__device__ __forceinline__ bool am_better(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}
__device__ __forceinline__ ArgMax am_wave(ArgMax a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(a.v, o, 64);
        const int oi = __shfl_xor(a.i, o, 64);
        if (am_better(ov, oi, a.v, a.i)) {
            a.v = ov;
            a.i = oi;
        }
    }
    return a;
}
__device__ __forceinline__ ArgMax am_block(const float* __restrict__ m, int n, float* sv, int* si) {
    ArgMax a{-INFINITY, 0x7fffffff};
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = m[i];
        if (am_better(v, i, a.v, a.i)) {
            a.v = v;
            a.i = i;
        }
    }
    a = am_wave(a);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) {
        sv[w] = a.v;
        si[w] = a.i;
    }
    __syncthreads();
    ArgMax r{sv[0], si[0]};
    for (int k = 1; k < nw; ++k)
        if (am_better(sv[k], si[k], r.v, r.i)) {
            r.v = sv[k];
            r.i = si[k];
        }
    return r;
}

__global__ void __launch_bounds__(256) k_argmax_decode(const float* __restrict__ hm, int32_t* __restrict__ index,
                                                       float* __restrict__ maxval, float* __restrict__ coords, int H, int W,
                                                       int mode) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int map = blockIdx.x;
    const float* m = hm + (size_t)map * H * W;
    const ArgMax r = am_block(m, H * W, sv, si);
    if (threadIdx.x != 0) return;
    if (index) index[map] = r.i;
    if (maxval) maxval[map] = r.v;
    if (!coords) return;
    const int x = r.i % W, y = r.i / W;
    float fx = (float)x, fy = (float)y;
    if (mode == 1) {  // quarter-pixel shift toward the larger neighbour; sign(0) = 0
        if (x > 0 && x < W - 1 && y > 0 && y < H - 1) {
            const float dx = m[y * W + x + 1] - m[y * W + x - 1], dy = m[(y + 1) * W + x] - m[(y - 1) * W + x];
            fx += 0.25f * (float)((dx > 0.f) - (dx < 0.f));
            fy += 0.25f * (float)((dy > 0.f) - (dy < 0.f));
        }
    } else if (mode == 2) {  // Taylor step, strict 1 < p < size-1, only where the 2nd difference is negative
        if (x > 1 && x < W - 1 && y > 1 && y < H - 1) {
            const float c = m[y * W + x];
            const float l = m[y * W + x - 1], rr = m[y * W + x + 1], u = m[(y - 1) * W + x], d = m[(y + 1) * W + x];
            const float dxx = (rr - 2.f * c) + l, dyy = (d - 2.f * c) + u;
            if (dxx < 0.f) fx += fminf(fmaxf((rr - l) / (2.f * fabsf(dxx)), -0.5f), 0.5f);
            if (dyy < 0.f) fy += fminf(fmaxf((d - u) / (2.f * fabsf(dyy)), -0.5f), 0.5f);
        }
    }
    coords[2 * map] = fx;
    coords[2 * map + 1] = fy;
}

extern "C" int pk_argmax_decode(const float* heatmaps, int32_t* index, float* maxval, float* coords, int BK, int H, int W,
                                int mode, void* stream) {
    PK_REQUIRE(heatmaps, "pk_argmax_decode: null heatmaps");
    PK_REQUIRE(map_shape_ok(BK, H, W), "pk_argmax_decode: bad shape");
    PK_REQUIRE(mode >= 0 && mode <= 2, "pk_argmax_decode: mode %d", mode);
    hipLaunchKernelGGL(k_argmax_decode, dim3(BK), dim3(256), 0, (hipStream_t)stream, heatmaps, index, maxval, coords, H, W, mode);
    return pk_launch_status("pk_argmax_decode");
}

// ================================================================================================ unbiased (DARK) decode
// Distribution-aware decoding: argmax, then one Newton step of the quadratic fitted to the logarithm of the Gaussian-smoothed map
// (include/posekernels.h states every operation; tests/unbiased_np.py restates it over the whole map).  The published form blurs the
// whole map and rescales it to the raw maximum before the logarithm; the rescale adds one constant to the log map, which cancels in every
// difference the step is made of, so it is dropped -- and without it only the 13 stencil points around the argmax need the blur.  Each
// heatmap element is therefore read from global memory ONCE, by am_block; the workgroup then blurs a (ksize + 4) x 5 patch: the row pass
// into LDS (one thread per entry, its ksize taps come back out of L2), the column pass at the 5 x 5 points, and lane 0 takes the step.
// Both passes fetch their operands UB_CHUNK at a time from addresses that are always valid (clamped; what lies outside is replaced by 0
// afterwards), so a chunk's loads are in flight together and only the fmaf chain is serial: this tail is latency, not bandwidth.
// The taps ride in the kernel arguments (no device table); every operation is rounded once, in a fixed order: the same bits on every run.
#define UB_MAX_K 31
#define UB_CHUNK 16
struct UbTaps {
    float v[UB_MAX_K];
};
__global__ void __launch_bounds__(256) k_unbiased_decode(const float* __restrict__ hm, UbTaps taps, int ksize, int32_t* __restrict__ index,
                                                         float* __restrict__ maxval, float* __restrict__ coords,
                                                         uint8_t* __restrict__ refined, int H, int W) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float sg[2 * UB_CHUNK];
    __shared__ float sR[(UB_MAX_K + 4) * 5];
    __shared__ float sL[25];
    const int map = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {      // static indices into the argument struct; am_block's barrier publishes sg
#pragma unroll
        for (int t = 0; t < 2 * UB_CHUNK; ++t) sg[t] = t < UB_MAX_K ? taps.v[t] : 0.0f;
    }
    const float* m = hm + (size_t)map * H * W;
    const ArgMax r = am_block(m, H * W, sv, si);
    const int px = r.i % W, py = r.i / W;
    if (tid == 0) {
        if (index) index[map] = r.i;
        if (maxval) maxval[map] = r.v;
    }
    if (!(px >= 2 && px <= W - 3 && py >= 2 && py <= H - 3)) {      // uniform over the workgroup: no stencil, no step
        if (tid == 0) {
            coords[2 * map] = (float)px;
            coords[2 * map + 1] = (float)py;
            if (refined) refined[map] = 0;
        }
        return;
    }
    const int c = (ksize - 1) / 2, rows = ksize + 4;
    // row pass: R[y][x] for y = py-2-c .. py+2+c, x = px-2 .. px+2; m counts as 0 outside the map (the tap is still multiplied in)
    for (int e = tid; e < rows * 5; e += blockDim.x) {
        const int rr = e / 5, y = py - 2 - c + rr, x0 = px - 2 + (e - rr * 5) - c;
        const bool row_in = y >= 0 && y < H;
        const float* mrow = m + min(max(y, 0), H - 1) * W;
        float acc = 0.0f;
        for (int t0 = 0; t0 < ksize; t0 += UB_CHUNK) {
            float v[UB_CHUNK], g[UB_CHUNK];
#pragma unroll
            for (int j = 0; j < UB_CHUNK; ++j) {
                const int x = x0 + t0 + j;
                g[j] = sg[t0 + j];
                const float raw = mrow[min(max(x, 0), W - 1)];
                // a bit mask, not a select: a select lets the compiler sink the load into a branch of its own and wait for each one
                const unsigned keep = 0u - (unsigned)(row_in & (x >= 0) & (x < W));
                v[j] = __uint_as_float(__float_as_uint(raw) & keep);
            }
#pragma unroll
            for (int j = 0; j < UB_CHUNK; ++j)
                if (t0 + j < ksize) acc = fmaf(g[j], v[j], acc);
        }
        sR[e] = acc;
    }
    __syncthreads();
    if (tid < 25) {      // column pass and logarithm at (py + tid/5 - 2, px + tid%5 - 2)
        const int ry = tid / 5, cx = tid - ry * 5;
        float acc = 0.0f;
        for (int t0 = 0; t0 < ksize; t0 += UB_CHUNK) {
            float v[UB_CHUNK], g[UB_CHUNK];
#pragma unroll
            for (int j = 0; j < UB_CHUNK; ++j) {
                g[j] = sg[t0 + j];
                v[j] = sR[(ry + min(t0 + j, ksize - 1)) * 5 + cx];
            }
#pragma unroll
            for (int j = 0; j < UB_CHUNK; ++j)
                if (t0 + j < ksize) acc = fmaf(g[j], v[j], acc);
        }
        sL[tid] = logf(fmaxf(acc, 1e-10f));
    }
    __syncthreads();
    if (tid != 0) return;
    auto L = [&](int dy, int dx) { return sL[(dy + 2) * 5 + dx + 2]; };
    const float two_l0 = __fmul_rn(2.0f, L(0, 0));
    const float dx = __fmul_rn(0.5f, __fsub_rn(L(0, 1), L(0, -1))), dy = __fmul_rn(0.5f, __fsub_rn(L(1, 0), L(-1, 0)));
    const float dxx = __fmul_rn(0.25f, __fadd_rn(__fsub_rn(L(0, 2), two_l0), L(0, -2)));
    const float dyy = __fmul_rn(0.25f, __fadd_rn(__fsub_rn(L(2, 0), two_l0), L(-2, 0)));
    const float dxy = __fmul_rn(0.25f, __fadd_rn(__fsub_rn(__fsub_rn(L(1, 1), L(-1, 1)), L(1, -1)), L(-1, -1)));
    const float det = __fsub_rn(__fmul_rn(dxx, dyy), __fmul_rn(dxy, dxy));
    const float ox = -__fdiv_rn(__fsub_rn(__fmul_rn(dyy, dx), __fmul_rn(dxy, dy)), det);
    const float oy = -__fdiv_rn(__fsub_rn(__fmul_rn(dxx, dy), __fmul_rn(dxy, dx)), det);
    // positive comparisons: a NaN anywhere fails them and the integers stand
    const bool step = dxx < 0.0f && det > 0.0f && fabsf(ox) <= 2.0f && fabsf(oy) <= 2.0f;
    coords[2 * map] = step ? __fadd_rn((float)px, ox) : (float)px;
    coords[2 * map + 1] = step ? __fadd_rn((float)py, oy) : (float)py;
    if (refined) refined[map] = step ? 1 : 0;
}

extern "C" int pk_unbiased_decode(const float* heatmaps, const float* taps_host, int ksize, int32_t* index, float* maxval, float* coords,
                                  uint8_t* refined, int BK, int H, int W, void* stream) {
    PK_REQUIRE(heatmaps && coords && taps_host, "pk_unbiased_decode: null pointer (heatmaps, coords and taps_host are required)");
    PK_REQUIRE(ksize >= 3 && ksize <= UB_MAX_K && (ksize & 1) == 1, "pk_unbiased_decode: ksize %d (odd, 3 to %d)", ksize, UB_MAX_K);
    PK_REQUIRE(map_shape_ok(BK, H, W), "pk_unbiased_decode: bad shape BK=%d H=%d W=%d", BK, H, W);
    UbTaps taps = {};
    for (int t = 0; t < ksize; ++t) taps.v[t] = taps_host[t];
    hipLaunchKernelGGL(k_unbiased_decode, dim3(BK), dim3(256), 0, (hipStream_t)stream, heatmaps, taps, ksize, index, maxval, coords, refined,
                       H, W);
    return pk_launch_status("pk_unbiased_decode");
}

// ================================================================================================ D1
__device__ __forceinline__ float bilinear_border(const float* __restrict__ p, int H, int W, float x, float y) {
    x = fminf(fmaxf(x, 0.f), (float)(W - 1));
    y = fminf(fmaxf(y, 0.f), (float)(H - 1));
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const float fx = x - (float)x0, fy = y - (float)y0;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);  // weight is 0 whenever the clamp bites
    return p[y0 * W + x0] * (1.f - fx) * (1.f - fy) + p[y0 * W + x1] * fx * (1.f - fy) + p[y1 * W + x0] * (1.f - fx) * fy +
           p[y1 * W + x1] * fx * fy;
}

__global__ void __launch_bounds__(256) k_softargmax_refine(const float* __restrict__ hm, const float* __restrict__ offsets,
                                                           const float* __restrict__ alpha_p, const float* __restrict__ fw_p,
                                                           float* __restrict__ coords, float* __restrict__ scores, int H, int W,
                                                           int radius) {
    __shared__ float red[16];
    const int map = blockIdx.x, n = H * W;
    const float* m = hm + (size_t)map * n;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, m[i]);
    mx = block_max(mx, red);
    float z = 0.f, sx = 0.f, sy = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float e = __expf(m[i] - mx);
        const int y = i / W;
        z += e;
        sx += e * (float)(i - y * W);
        sy += e * (float)y;
    }
    z = block_sum(z, red);
    sx = block_sum(sx, red);
    sy = block_sum(sy, red);
    if (threadIdx.x != 0) return;
    const float gx = sx / z, gy = sy / z;
    // local softmax centroid of the clipped (2r+1)^2 patch around round-half-even(global)
    const int px = (int)fminf(fmaxf(rintf(gx), 0.f), (float)(W - 1)), py = (int)fminf(fmaxf(rintf(gy), 0.f), (float)(H - 1));
    const int x0 = max(0, px - radius), x1 = min(W, px + radius + 1), y0 = max(0, py - radius), y1 = min(H, py + radius + 1);
    float lm = -INFINITY;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) lm = fmaxf(lm, m[y * W + x]);
    float lz = 0.f, lx = 0.f, ly = 0.f;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const float e = __expf(m[y * W + x] - lm);
            lz += e;
            lx += e * (float)x;
            ly += e * (float)y;
        }
    const float a = 1.f / (1.f + __expf(-alpha_p[0]));
    float cx = a * gx + (1.f - a) * (lx / lz), cy = a * gy + (1.f - a) * (ly / lz);
    if (offsets) {
        const float fw = 1.f / (1.f + __expf(-fw_p[0]));
        const float* o = offsets + (size_t)map * 2 * n;
        const float ox = bilinear_border(o, H, W, cx, cy), oy = bilinear_border(o + n, H, W, cx, cy);
        cx += fw * ox;
        cy += fw * oy;
    }
    coords[2 * map] = cx;
    coords[2 * map + 1] = cy;
    scores[map] = mx;
}

extern "C" int pk_softargmax_refine_decode(const float* heatmaps, const float* offsets, const float* alpha_param,
                                           const float* fusion_weight_param, float* coords, float* scores, int BK, int H, int W,
                                           int local_radius, void* stream) {
    PK_REQUIRE(heatmaps && alpha_param && coords && scores, "pk_softargmax_refine_decode: null pointer");
    PK_REQUIRE(!offsets || fusion_weight_param, "pk_softargmax_refine_decode: offsets given without fusion_weight");
    PK_REQUIRE(BK > 0 && H > 0 && W > 0 && local_radius >= 0, "pk_softargmax_refine_decode: bad shape");
    hipLaunchKernelGGL(k_softargmax_refine, dim3(BK), dim3(256), 0, (hipStream_t)stream, heatmaps, offsets, alpha_param,
                       fusion_weight_param, coords, scores, H, W, local_radius);
    return pk_launch_status("pk_softargmax_refine_decode");
}

// LocalGaussianRefinement.forward (fusion_head.py:74-128) about coordinates handed in by the caller: softmax-weighted centroid of the
// clipped (2r+1)^2 patch around clamp(round_half_even(c)).  One lane per map (25 pixels).
__global__ void k_local_refine(const float* __restrict__ hm, const float* __restrict__ cin, float* __restrict__ cout, int BK, int H,
                               int W, int radius) {
    const int map = blockIdx.x * blockDim.x + threadIdx.x;
    if (map >= BK) return;
    const float* m = hm + (size_t)map * H * W;
    const int px = (int)fminf(fmaxf(rintf(cin[2 * map]), 0.f), (float)(W - 1)), py = (int)fminf(fmaxf(rintf(cin[2 * map + 1]), 0.f), (float)(H - 1));
    const int x0 = max(0, px - radius), x1 = min(W, px + radius + 1), y0 = max(0, py - radius), y1 = min(H, py + radius + 1);
    float lm = -INFINITY;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) lm = fmaxf(lm, m[y * W + x]);
    float lz = 0.f, lx = 0.f, ly = 0.f;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const float e = __expf(m[y * W + x] - lm);
            lz += e;
            lx += e * (float)x;
            ly += e * (float)y;
        }
    cout[2 * map] = lx / lz;
    cout[2 * map + 1] = ly / lz;
}
extern "C" int pk_local_gaussian_refine(const float* heatmaps, const float* coords_in, float* coords_out, int BK, int H, int W,
                                        int local_radius, void* stream) {
    PK_REQUIRE(heatmaps && coords_in && coords_out && BK > 0 && H > 0 && W > 0 && local_radius >= 0, "pk_local_gaussian_refine: bad argument");
    hipLaunchKernelGGL(k_local_refine, dim3((BK + 255) / 256), dim3(256), 0, (hipStream_t)stream, heatmaps, coords_in, coords_out, BK, H, W,
                       local_radius);
    return pk_launch_status("pk_local_gaussian_refine");
}

// Backward of SoftArgmax2D.forward (fusion_head.py:24-71): coords = sum softmax(h) (x, y), scores = max h.
//   d h_i = p_i ((x_i - c_x) g_cx + (y_i - c_y) g_cy) + g_score [i == first arg max]
__global__ void __launch_bounds__(256) k_softargmax_bwd(const float* __restrict__ hm, const float* __restrict__ coords,
                                                        const float* __restrict__ scores, const float* __restrict__ gco,
                                                        const float* __restrict__ gsc, float* __restrict__ dhm, int H, int W) {
    __shared__ float red[16];
    __shared__ int first;
    const int map = blockIdx.x, n = H * W;
    const float* m = hm + (size_t)map * n;
    const float mx = scores[map], cx = coords[2 * map], cy = coords[2 * map + 1];
    float z = 0.f;
    int arg = n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = m[i];
        z += __expf(v - mx);
        if (v == mx && i < arg) arg = i;
    }
    z = block_sum(z, red);
    if (threadIdx.x == 0) first = n;
    __syncthreads();
    atomicMin(&first, arg);
    __syncthreads();
    const float zinv = 1.f / z, gx = gco ? gco[2 * map] : 0.f, gy = gco ? gco[2 * map + 1] : 0.f, gs = gsc ? gsc[map] : 0.f;
    float* d = dhm + (size_t)map * n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int y = i / W;
        const float p = __expf(m[i] - mx) * zinv;
        d[i] = p * (((float)(i - y * W) - cx) * gx + ((float)y - cy) * gy) + (i == first ? gs : 0.f);
    }
}
extern "C" int pk_softargmax_bwd(const float* heatmaps, const float* coords, const float* scores, const float* grad_coords,
                                 const float* grad_scores, float* d_heatmaps, int BK, int H, int W, void* stream) {
    PK_REQUIRE(heatmaps && coords && scores && d_heatmaps && BK > 0 && H > 0 && W > 0, "pk_softargmax_bwd: bad argument");
    hipLaunchKernelGGL(k_softargmax_bwd, dim3(BK), dim3(256), 0, (hipStream_t)stream, heatmaps, coords, scores, grad_coords, grad_scores,
                       d_heatmaps, H, W);
    return pk_launch_status("pk_softargmax_bwd");
}

// ================================================================================================ D3 tail
__global__ void k_window_refine(const float* __restrict__ hm, const float* __restrict__ cin, float* __restrict__ cout, int BK,
                                int H, int W, int window) {
    const int map = blockIdx.x * blockDim.x + threadIdx.x;
    if (map >= BK) return;
    const float* m = hm + (size_t)map * H * W;
    const int hw = window / 2;
    const int x = (int)cin[2 * map], y = (int)cin[2 * map + 1];  // int() truncation
    const int x0 = max(0, x - hw), x1 = min(W, x + hw + 1), y0 = max(0, y - hw), y1 = min(H, y + hw + 1);
    float ox = cin[2 * map], oy = cin[2 * map + 1];
    if (x1 > x0 && y1 > y0) {
        float s = 0.f, ax = 0.f, ay = 0.f;
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) {
                const float v = m[yy * W + xx];
                s += v;
                ax += v * (float)xx;
                ay += v * (float)yy;
            }
        ox = ax / (s + 1e-8f);
        oy = ay / (s + 1e-8f);
    }
    cout[2 * map] = ox;
    cout[2 * map + 1] = oy;
}
extern "C" int pk_window_refine(const float* heatmaps, const float* coords_in, float* coords_out, int BK, int H, int W,
                                int window, void* stream) {
    PK_REQUIRE(heatmaps && coords_in && coords_out && BK > 0 && H > 0 && W > 0 && window > 0, "pk_window_refine: bad argument");
    hipLaunchKernelGGL(k_window_refine, dim3((BK + 255) / 256), dim3(256), 0, (hipStream_t)stream, heatmaps, coords_in, coords_out,
                       BK, H, W, window);
    return pk_launch_status("pk_window_refine");
}

// fused_decode tail: hp scaled by (sx,sy); if regression given: a = mv/(mv+0.1); out = a*hp + (1-a)*reg*reg_scale
__global__ void k_fused_blend(const float* __restrict__ hp, const float* __restrict__ mv, const float* __restrict__ reg,
                              float* __restrict__ out, int BK, float sx, float sy, float reg_scale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK) return;
    const float hx = hp[2 * i] * sx, hy = hp[2 * i + 1] * sy;
    if (reg) {
        const float a = mv[i] / (mv[i] + 0.1f);
        out[2 * i] = a * hx + (1.f - a) * (reg[2 * i] * reg_scale);
        out[2 * i + 1] = a * hy + (1.f - a) * (reg[2 * i + 1] * reg_scale);
    } else {
        out[2 * i] = hx;
        out[2 * i + 1] = hy;
    }
}
extern "C" int pk_fused_blend(const float* hp, const float* maxvals, const float* regression, float* out, int BK, float sx,
                              float sy, float reg_scale, void* stream) {
    PK_REQUIRE(hp && out && BK > 0 && (!regression || maxvals), "pk_fused_blend: bad argument");
    hipLaunchKernelGGL(k_fused_blend, dim3((BK + 255) / 256), dim3(256), 0, (hipStream_t)stream, hp, maxvals, regression, out, BK,
                       sx, sy, reg_scale);
    return pk_launch_status("pk_fused_blend");
}

__global__ void k_affine_coords(const float* __restrict__ c, const float* __restrict__ center, const float* __restrict__ scale,
                                float* __restrict__ out, int B, int K, float mx, float my, const float* __restrict__ mvals,
                                float thr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * K) return;
    const int b = i / K;
    const float keep = mvals ? (mvals[i] > thr ? 1.f : 0.f) : 1.f;
    out[2 * i] = (c[2 * i] * keep) * (scale[2 * b] * mx) + center[2 * b] - scale[2 * b] * 0.5f;
    out[2 * i + 1] = (c[2 * i + 1] * keep) * (scale[2 * b + 1] * my) + center[2 * b + 1] - scale[2 * b + 1] * 0.5f;
}
extern "C" int pk_affine_coords(const float* coords, const float* center, const float* scale, float* out, int B, int K,
                                float mul_x, float mul_y, const float* mask_maxvals, float threshold, void* stream) {
    PK_REQUIRE(coords && center && scale && out && B > 0 && K > 0, "pk_affine_coords: bad argument");
    hipLaunchKernelGGL(k_affine_coords, dim3((B * K + 255) / 256), dim3(256), 0, (hipStream_t)stream, coords, center, scale, out, B,
                       K, mul_x, mul_y, mask_maxvals, threshold);
    return pk_launch_status("pk_affine_coords");
}

// ================================================================================================ D4
__global__ void __launch_bounds__(256) k_flip_merge(const float* __restrict__ a, const float* __restrict__ bf,
                                                    const int32_t* __restrict__ partner, float* __restrict__ out, int K, int H,
                                                    int W) {
    const int map = blockIdx.x, b = map / K, k = map - b * K;
    const float* pa = a + (size_t)map * H * W;
    const float* pb = bf + ((size_t)b * K + partner[k]) * H * W;
    float* po = out + (size_t)map * H * W;
    for (int i = threadIdx.x; i < H * W; i += blockDim.x) {
        const int y = i / W, x = i - y * W;
        po[i] = (pa[i] + pb[y * W + (W - 1 - x)]) / 2.f;
    }
}
extern "C" int pk_flip_merge(const float* a, const float* b_flipped, const int32_t* partner, float* out, int B, int K, int H,
                             int W, void* stream) {
    PK_REQUIRE(a && b_flipped && partner && out && B > 0 && K > 0 && H > 0 && W > 0, "pk_flip_merge: bad argument");
    hipLaunchKernelGGL(k_flip_merge, dim3(B * K), dim3(256), 0, (hipStream_t)stream, a, b_flipped, partner, out, K, H, W);
    return pk_launch_status("pk_flip_merge");
}

// ------------------------------------------------------------------------------------------------ D4 over several crop scales
// Multi-scale flip test: S crops of the same centre with box scale s * scale, each run plain (f = 0) and mirrored (f = 1), brought back
// into the frame of the scale-1.0 crop and averaged.  Base heat-px u is seen by pass s at u_s = W/2 + (u - W/2) / s (pk_affine_coords'
// convention: img = u * scale / W + centre - scale / 2); the pass is sampled there bilinearly if u_s lies on its map (borders included),
// otherwise it contributes nothing and the divisor shrinks with it.  One workgroup per (b, k) map like k_flip_merge; the S * F source
// maps are gathered from global memory (every map is consumed whole, so L2 serves the four taps; 6 maps of 96 x 72 do not fit in LDS).
// Every operation is written out with one rounding each and in a fixed order (s ascending, f = 0 before f = 1): no atomics, the same
// bits on every run, and tests/multiscale_np.py can restate it.  The 1 / s table rides in the kernel arguments (no device table).
struct MsInv {
    float v[8];
};
__device__ __forceinline__ float ms_lerp(float a, float b, float t) { return fmaf(t, __fsub_rn(b, a), a); }
template <int S>
__global__ void __launch_bounds__(256) k_multiscale_merge(const float* __restrict__ stack, const int32_t* __restrict__ partner,
                                                          float* __restrict__ out, MsInv inv, int F, int B, int K, int H, int W) {
    const int map = blockIdx.x, b = map / K, k = map - b * K, n = H * W;
    const int kf = F == 2 ? partner[k] : k;
    const float cx = 0.5f * (float)W, cy = 0.5f * (float)H, xmax = (float)(W - 1), ymax = (float)(H - 1);
    float* po = out + (size_t)map * n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int y = i / W, x = i - y * W;
        float acc = 0.f;
        int cnt = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float us = fmaf(__fsub_rn((float)x, cx), inv.v[s], cx), vs = fmaf(__fsub_rn((float)y, cy), inv.v[s], cy);
            if (!(us >= 0.f && us <= xmax && vs >= 0.f && vs <= ymax)) continue;
            const int x0 = (int)floorf(us), y0 = (int)floorf(vs);
            const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
            const float lx = __fsub_rn(us, (float)x0), ly = __fsub_rn(vs, (float)y0);
            const float* m = stack + (((size_t)s * F * B + b) * K + k) * n;
            acc = __fadd_rn(acc, ms_lerp(ms_lerp(m[y0 * W + x0], m[y0 * W + x1], lx), ms_lerp(m[y1 * W + x0], m[y1 * W + x1], lx), ly));
            ++cnt;
            if (F == 2) {       // the mirrored crop's map: partner channel, mirrored columns, same weights (no one-pixel shift)
                const float* mf = stack + ((((size_t)s * F + 1) * B + b) * K + kf) * n;
                const int c0 = W - 1 - x0, c1 = W - 1 - x1;
                acc = __fadd_rn(acc, ms_lerp(ms_lerp(mf[y0 * W + c0], mf[y0 * W + c1], lx), ms_lerp(mf[y1 * W + c0], mf[y1 * W + c1], lx), ly));
                ++cnt;
            }
        }
        po[i] = cnt > 0 ? __fdiv_rn(acc, (float)cnt) : 0.f;
    }
}
template <int S>
static void multiscale_merge_launch(const float* stack, const int32_t* partner, float* out, const MsInv& inv, int F, int B, int K, int H, int W,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(k_multiscale_merge<S>, dim3(B * K), dim3(256), 0, stream, stack, partner, out, inv, F, B, K, H, W);
}
extern "C" int pk_multiscale_merge(const float* stack, const int32_t* partner, const float* inv_scales_host, float* out, int S, int F, int B,
                                   int K, int H, int W, void* stream) {
    PK_REQUIRE(stack && inv_scales_host && out, "pk_multiscale_merge: null pointer");
    PK_REQUIRE(F == 1 || F == 2, "pk_multiscale_merge: F = %d passes per scale (1: plain, 2: plain + mirrored)", F);
    PK_REQUIRE(F == 1 || partner, "pk_multiscale_merge: the mirrored passes need the partner table");
    PK_REQUIRE(S >= 1 && S <= 8, "pk_multiscale_merge: %d scales (1 to 8)", S);
    PK_REQUIRE(K > 0 && (int64_t)B * K < 0x7fffffff && map_shape_ok(B, H, W), "pk_multiscale_merge: bad shape B=%d K=%d H=%d W=%d", B, K, H, W);
    MsInv inv = {};
    for (int s = 0; s < S; ++s) {
        PK_REQUIRE(inv_scales_host[s] > 0.f && inv_scales_host[s] < INFINITY, "pk_multiscale_merge: inverse scale %d is %g (finite, > 0)", s,
                   (double)inv_scales_host[s]);
        inv.v[s] = inv_scales_host[s];
    }
    const hipStream_t st = (hipStream_t)stream;
    switch (S) {
        case 1: multiscale_merge_launch<1>(stack, partner, out, inv, F, B, K, H, W, st); break;
        case 2: multiscale_merge_launch<2>(stack, partner, out, inv, F, B, K, H, W, st); break;
        case 3: multiscale_merge_launch<3>(stack, partner, out, inv, F, B, K, H, W, st); break;
        case 4: multiscale_merge_launch<4>(stack, partner, out, inv, F, B, K, H, W, st); break;
        case 5: multiscale_merge_launch<5>(stack, partner, out, inv, F, B, K, H, W, st); break;
        case 6: multiscale_merge_launch<6>(stack, partner, out, inv, F, B, K, H, W, st); break;
        case 7: multiscale_merge_launch<7>(stack, partner, out, inv, F, B, K, H, W, st); break;
        default: multiscale_merge_launch<8>(stack, partner, out, inv, F, B, K, H, W, st); break;
    }
    return pk_launch_status("pk_multiscale_merge");
}
