// Pose overlays drawn on the device (utils/visualization.py): skeletons and boxes rasterised with exact integer coverage, and the
// heatmap overlay (max over joints, bilinear resize, per-image normalisation, colour LUT, integer blend).
//
// Rasterisation rule of pk_draw_shapes ("Drawing on the device").  One unit is 1/8 pixel; a coordinate x becomes
// rint(8 x) after clamping to [-8192, 16384] px.  Pixel (x, y) has its centre at (x, y) and carries 16 samples at
// 8x + {-3,-1,1,3}, 8y + {-3,-1,1,3}; the coverage n of a shape is the number of samples inside it, and the shape is composited as
// c <- (c (16 - n) + colour n + 8) >> 4, shape after shape in painter's order.  Every inside test is integer arithmetic, so the
// bits are the same on any machine and equal tests/draw_np.py.
#include "pk_common.h"

#define DRAW_TW 32            // tile: 32 x 8 pixels, one per thread (a row of a tile is 96 contiguous bytes)
#define DRAW_TH 8
#define DRAW_CAP 512          // shape records held in LDS at a time (10 KiB); more survivors are drawn in several passes, in order
#define DRAW_MAX_SIZE 64      // point_radius, line_thickness, box thickness
#define DRAW_MAX_HW 8192

enum { SH_BOX = 0, SH_LIMB = 1, SH_JOINT = 2 };

struct DrawArgs {
    uint8_t* img;
    int N, H, W;
    const float* poses;
    const float* scores;
    const int32_t* pose_img;
    int P, K;
    const int32_t* limbs;
    int L;
    const uint8_t* colors;
    int C;
    const float* boxes;
    const int32_t* box_img;
    int Q;
    uint32_t box_color;       // channel 0 in bits 0-7, 1 in 8-15, 2 in 16-23
    int box_half;             // 4 * thickness: half the line width in units
    float thr;
    int r0, r1, half;         // 8 r, 8 (r + 1), 4 * line_thickness
};

__device__ __forceinline__ bool draw_quant(float v, int& q) {
    if (!(fabsf(v) < INFINITY)) return false;                     // NaN and +-inf: not drawn
    q = (int)rintf(8.f * fminf(fmaxf(v, -8192.f), 16384.f));      // exact: a power-of-two scale, then round half to even
    return true;
}
__device__ __forceinline__ bool draw_joint(const DrawArgs& a, int p, int k, int& x, int& y) {
    const float s = a.scores[(size_t)p * a.K + k];
    if (!(fabsf(s) < INFINITY) || !(s >= a.thr)) return false;
    return draw_quant(a.poses[((size_t)p * a.K + k) * 2], x) && draw_quant(a.poses[((size_t)p * a.K + k) * 2 + 1], y);
}
__device__ __forceinline__ uint32_t draw_color(const DrawArgs& a, int k) {
    const uint8_t* c = a.colors + (size_t)(k % a.C) * 3;
    return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
}
// first index with v[i] >= key in a non-decreasing table
__device__ __forceinline__ int draw_lower_bound(const int32_t* v, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Candidate `idx` of an image in painter's order: its boxes, then per pose the limbs in table order and the joints in index order.
// Returns whether it is drawn at all, its record and its bounding box in units (expanded by its width).
__device__ __forceinline__ bool draw_candidate(const DrawArgs& a, int idx, int b_lo, int n_box, int p_lo, int4& g, uint32_t& kc,
                                               int& bx0, int& by0, int& bx1, int& by1) {
    if (idx < n_box) {
        const float* b = a.boxes + (size_t)(b_lo + idx) * 4;
        if (!(draw_quant(b[0], g.x) && draw_quant(b[1], g.y) && draw_quant(b[2], g.z) && draw_quant(b[3], g.w))) return false;
        kc = ((uint32_t)SH_BOX << 24) | a.box_color;
        bx0 = g.x - a.box_half; by0 = g.y - a.box_half; bx1 = g.z + a.box_half; by1 = g.w + a.box_half;
        return true;
    }
    idx -= n_box;
    const int per = a.L + a.K, p = p_lo + idx / per, s = idx % per;
    if (s < a.L) {
        const int ja = a.limbs[2 * s], jb = a.limbs[2 * s + 1];
        if (ja < 0 || jb < 0 || ja >= a.K || jb >= a.K) return false;
        if (!(draw_joint(a, p, ja, g.x, g.y) && draw_joint(a, p, jb, g.z, g.w))) return false;
        kc = ((uint32_t)SH_LIMB << 24) | draw_color(a, ja);
        bx0 = min(g.x, g.z) - a.half; bx1 = max(g.x, g.z) + a.half; by0 = min(g.y, g.w) - a.half; by1 = max(g.y, g.w) + a.half;
        return true;
    }
    const int k = s - a.L;
    if (!draw_joint(a, p, k, g.x, g.y)) return false;
    g.z = g.w = 0;
    kc = ((uint32_t)SH_JOINT << 24) | draw_color(a, k);
    bx0 = g.x - a.r1; bx1 = g.x + a.r1; by0 = g.y - a.r1; by1 = g.y + a.r1;
    return true;
}

__device__ __forceinline__ void draw_blend(int (&col)[3], uint32_t colour, int n) {
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = (col[c] * (16 - n) + (int)((colour >> (8 * c)) & 255u) * n + 8) >> 4;
}

// Coverage of one record at the pixel whose centre is (sx, sy) units, composited into col.  Returns whether a sample was covered.
__device__ __forceinline__ bool draw_apply(const DrawArgs& a, const int4 g, const uint32_t kc, const int sx, const int sy, int (&col)[3]) {
    const int kind = (int)(kc >> 24);
    if (kind == SH_JOINT) {
        if (abs(sx - g.x) > a.r1 + 3 || abs(sy - g.y) > a.r1 + 3) return false;
        const int q0 = a.r0 * a.r0, q1 = a.r1 * a.r1;
        int nd = 0, nr = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int dx = sx + 2 * i - 3 - g.x, dy = sy + 2 * j - 3 - g.y, d = dx * dx + dy * dy;   // |dx| <= 8 * 65 + 6
                nd += d <= q0;
                nr += d > q0 && d <= q1;
            }
        draw_blend(col, kc, nd);
        draw_blend(col, 0xffffffu, nr);
        return (nd | nr) != 0;
    }
    if (kind == SH_LIMB) {
        if (sx + 3 < min(g.x, g.z) - a.half || sx - 3 > max(g.x, g.z) + a.half || sy + 3 < min(g.y, g.w) - a.half ||
            sy - 3 > max(g.y, g.w) + a.half)
            return false;
        const long long ex = g.z - g.x, ey = g.w - g.y, lq = ex * ex + ey * ey, h2 = (long long)a.half * a.half;
        int n = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long wx = sx + 2 * i - 3 - g.x, wy = sy + 2 * j - 3 - g.y, s = wx * ex + wy * ey;
                bool in;
                if (lq == 0 || s <= 0) {
                    in = wx * wx + wy * wy <= h2;
                } else if (s >= lq) {
                    const long long vx = wx - ex, vy = wy - ey;
                    in = vx * vx + vy * vy <= h2;
                } else {
                    // |w x e| < 2^32 or the sample is outside (h^2 Lq < 2^64); then the square fits unsigned 64 bits
                    const long long cr = wx * ey - wy * ex;
                    const unsigned long long m = (unsigned long long)(cr < 0 ? -cr : cr);
                    in = m < (1ull << 32) && m * m <= (unsigned long long)h2 * (unsigned long long)lq;
                }
                n += in;
            }
        draw_blend(col, kc, n);
        return n != 0;
    }
    // box: inside the outer rectangle and not strictly inside the inner one; both separable, and inner is a subset of outer
    const int hb = a.box_half;
    if (sx + 3 < g.x - hb || sx - 3 > g.z + hb || sy + 3 < g.y - hb || sy - 3 > g.w + hb) return false;
    int ox = 0, oy = 0, ix = 0, iy = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = sx + 2 * i - 3, y = sy + 2 * i - 3;
        ox += x >= g.x - hb && x <= g.z + hb;
        oy += y >= g.y - hb && y <= g.w + hb;
        ix += x > g.x + hb && x < g.z - hb;
        iy += y > g.y + hb && y < g.w - hb;
    }
    const int n = ox * oy - ix * iy;
    draw_blend(col, kc, n);
    return n != 0;
}

// Gather over image tiles: a workgroup owns a 32 x 8 tile of one image.  It walks the image's candidates in painter's order 256 at a
// time, keeps those whose expanded bounding box meets the tile (ordered compaction: wave ballots and a prefix over the four waves, so
// the list in LDS is in painter's order), and every thread composites the list into its own pixel, held in registers.  No shape is
// split across workgroups and nothing is accumulated through memory: the order, and so the bits, are fixed.  A tile that no shape
// reaches neither reads nor writes the image.
__global__ void __launch_bounds__(256) k_draw_shapes(const DrawArgs a) {
    __shared__ int4 s_geo[DRAW_CAP];
    __shared__ uint32_t s_kc[DRAW_CAP];
    __shared__ int s_wcnt[4];
    const int img = blockIdx.z, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int tx0 = blockIdx.x * DRAW_TW, ty0 = blockIdx.y * DRAW_TH;
    const int px = tx0 + (t & (DRAW_TW - 1)), py = ty0 + t / DRAW_TW;
    const bool live = px < a.W && py < a.H;
    const int ux0 = 8 * tx0 - 3, ux1 = 8 * min(tx0 + DRAW_TW - 1, a.W - 1) + 3;
    const int uy0 = 8 * ty0 - 3, uy1 = 8 * min(ty0 + DRAW_TH - 1, a.H - 1) + 3;
    const int b_lo = a.Q > 0 ? draw_lower_bound(a.box_img, a.Q, img) : 0;
    const int n_box = a.Q > 0 ? draw_lower_bound(a.box_img, a.Q, img + 1) - b_lo : 0;
    const int p_lo = a.P > 0 ? draw_lower_bound(a.pose_img, a.P, img) : 0;
    const int n_pose = a.P > 0 ? draw_lower_bound(a.pose_img, a.P, img + 1) - p_lo : 0;
    const int total = n_box + n_pose * (a.L + a.K);
    if (total <= 0) return;
    uint8_t* pix = a.img + (((size_t)img * a.H + (live ? py : 0)) * a.W + (live ? px : 0)) * 3;
    int col[3] = {0, 0, 0};
    bool loaded = false, dirty = false;
    int count = 0;
    for (int base = 0; base < total; base += 256) {
        const int idx = base + t;
        int4 g = make_int4(0, 0, 0, 0);
        uint32_t kc = 0;
        bool keep = false;
        if (idx < total) {
            int bx0, by0, bx1, by1;
            keep = draw_candidate(a, idx, b_lo, n_box, p_lo, g, kc, bx0, by0, bx1, by1) && bx0 <= ux1 && bx1 >= ux0 && by0 <= uy1 && by1 >= uy0;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wcnt[wv] = __popcll(m);
        __syncthreads();
        int off = count, tot = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = s_wcnt[i];
            off += i < wv ? c : 0;
            tot += c;
        }
        if (keep) {
            const int at = off + __popcll(m & ((1ull << lane) - 1ull));      // < count + 256 <= DRAW_CAP
            s_geo[at] = g;
            s_kc[at] = kc;
        }
        count += tot;
        __syncthreads();
        if (count > DRAW_CAP - 256 || base + 256 >= total) {
            if (count > 0 && live) {
                if (!loaded) {
                    col[0] = pix[0]; col[1] = pix[1]; col[2] = pix[2];
                    loaded = true;
                }
                for (int i = 0; i < count; ++i) dirty |= draw_apply(a, s_geo[i], s_kc[i], 8 * px, 8 * py, col);
            }
            count = 0;
            __syncthreads();
        }
    }
    if (dirty) {
        pix[0] = (uint8_t)col[0]; pix[1] = (uint8_t)col[1]; pix[2] = (uint8_t)col[2];
    }
}

extern "C" int pk_draw_shapes(void* images_u8, int N, int H, int W, const float* poses, const float* scores, const int32_t* image_index, int P,
                              int K, const int32_t* limbs, int L, const void* colors_u8, int C, const float* boxes,
                              const int32_t* box_image_index, int Q, int box_c0, int box_c1, int box_c2, int box_thickness,
                              float score_threshold, int point_radius, int line_thickness, void* stream) {
    PK_REQUIRE(images_u8, "pk_draw_shapes: null image pointer");
    PK_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "pk_draw_shapes: bad batch shape N=%d H=%d W=%d", N, H, W);
    PK_REQUIRE(H <= DRAW_MAX_HW && W <= DRAW_MAX_HW, "pk_draw_shapes: images up to %d x %d (got %d x %d)", DRAW_MAX_HW, DRAW_MAX_HW, H, W);
    PK_REQUIRE(P >= 0 && Q >= 0 && L >= 0 && K >= 0, "pk_draw_shapes: negative count");
    PK_REQUIRE(point_radius >= 0 && point_radius <= DRAW_MAX_SIZE && line_thickness >= 1 && line_thickness <= DRAW_MAX_SIZE,
               "pk_draw_shapes: point_radius 0..%d and line_thickness 1..%d (got %d, %d)", DRAW_MAX_SIZE, DRAW_MAX_SIZE, point_radius, line_thickness);
    if (P > 0) {
        PK_REQUIRE(poses && scores && image_index && colors_u8, "pk_draw_shapes: null pose pointer");
        PK_REQUIRE(K > 0 && C > 0 && (L == 0 || limbs), "pk_draw_shapes: bad pose tables K=%d C=%d L=%d", K, C, L);
    }
    if (Q > 0) {
        PK_REQUIRE(boxes && box_image_index, "pk_draw_shapes: null box pointer");
        PK_REQUIRE(box_thickness >= 1 && box_thickness <= DRAW_MAX_SIZE, "pk_draw_shapes: box thickness 1..%d (got %d)", DRAW_MAX_SIZE, box_thickness);
        PK_REQUIRE((box_c0 | box_c1 | box_c2) >= 0 && (box_c0 | box_c1 | box_c2) <= 255, "pk_draw_shapes: box colour outside 0..255");
    }
    PK_REQUIRE((int64_t)P * ((int64_t)L + K) + Q < (int64_t)1 << 30, "pk_draw_shapes: too many shapes");
    if (P == 0 && Q == 0) return PK_OK;
    DrawArgs a;
    a.img = (uint8_t*)images_u8; a.N = N; a.H = H; a.W = W;
    a.poses = poses; a.scores = scores; a.pose_img = image_index; a.P = P; a.K = P > 0 ? K : 0;
    a.limbs = limbs; a.L = P > 0 ? L : 0; a.colors = (const uint8_t*)colors_u8; a.C = C;
    a.boxes = boxes; a.box_img = box_image_index; a.Q = Q;
    a.box_color = (uint32_t)box_c0 | ((uint32_t)box_c1 << 8) | ((uint32_t)box_c2 << 16);
    a.box_half = 4 * box_thickness;
    a.thr = score_threshold;
    a.r0 = 8 * point_radius; a.r1 = 8 * (point_radius + 1); a.half = 4 * line_thickness;
    hipLaunchKernelGGL(k_draw_shapes, dim3((W + DRAW_TW - 1) / DRAW_TW, (H + DRAW_TH - 1) / DRAW_TH, N), dim3(256), 0, (hipStream_t)stream, a);
    return pk_launch_status("pk_draw_shapes");
}

// ================================================================================================ heatmap overlay
// draw_heatmaps of the reference (utils/visualization.py:93-127) for a batch: m = max over the K maps; m resized bilinearly to (H, W)
// with the exchange units' half-pixel rule (bil_taps of pk_exchange.hip restated); per-image min / max of the RESIZED plane (per-workgroup
// partials, fixed-order finish: no atomics); v = (m - min) / (max - min + 1e-8); idx = floor(255 v); colour = LUT[idx];
// out = (img (256 - a) + colour a + 128) >> 8 with a = clamp(rint(256 alpha), 0, 256).  The resize is evaluated twice (statistics pass
// and blend pass) by the same function, so both passes see the same bits; the resized plane is never stored.
__device__ __forceinline__ void ov_taps(int o, int n_in, int n_out, int& i0, int& i1, float& f) {
    float s = ((float)o + 0.5f) * ((float)n_in / (float)n_out) - 0.5f;
    s = fmaxf(s, 0.f);
    i0 = min((int)s, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    f = s - (float)i0;
}
__device__ __forceinline__ float ov_bilinear(const float* __restrict__ m, int w, int y0, int y1, int x0, int x1, float fy, float fx) {
    return (m[y0 * w + x0] * (1.f - fx) + m[y0 * w + x1] * fx) * (1.f - fy) + (m[y1 * w + x0] * (1.f - fx) + m[y1 * w + x1] * fx) * fy;
}
__device__ __forceinline__ float ov_resized(const float* __restrict__ m, int h, int w, int H, int W, int y, int x) {
    int y0, y1, x0, x1;
    float fy, fx;
    ov_taps(y, h, H, y0, y1, fy);
    ov_taps(x, w, W, x0, x1, fx);
    return ov_bilinear(m, w, y0, y1, x0, x1, fy, fx);
}
static inline int ov_blocks(int H, int W) {
    const int64_t n = ((int64_t)H * W + 2047) / 2048;
    return (int)(n < 1 ? 1 : (n > 256 ? 256 : n));
}

__global__ void __launch_bounds__(256) k_overlay_max(const float* __restrict__ hm, float* __restrict__ m, int K, int hw) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (i >= hw) return;
    const float* p = hm + (size_t)n * K * hw + i;
    float v = p[0];
    for (int k = 1; k < K; ++k) v = fmaxf(v, p[(size_t)k * hw]);
    m[(size_t)n * hw + i] = v;
}
// Minimum of `lo` and maximum of `hi` over the 256 threads of the block, stored by thread 0 as the pair at `at()` (evaluated in that
// thread alone): the xor butterfly inside the wave, one LDS slot per wave, the four waves as (0, 1), (2, 3).  fminf / fmaxf, not a
// comparison: they ignore a NaN.  One barrier: a kernel calls it once.
template <class At>
__device__ __forceinline__ void ov_block_minmax_store(float lo, float hi, At at) {
    __shared__ float s_lo[4], s_hi[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* out = at();
        out[0] = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
        out[1] = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
    }
}
__global__ void __launch_bounds__(256) k_overlay_minmax(const float* __restrict__ mplane, float* __restrict__ partial, int h, int w, int H, int W) {
    const int n = blockIdx.y, total = H * W;
    const float* m = mplane + (size_t)n * h * w;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int y = i / W;
        const float v = ov_resized(m, h, w, H, W, y, i - y * W);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    ov_block_minmax_store(lo, hi, [&] { return partial + ((size_t)n * gridDim.x + blockIdx.x) * 2; });
}
__global__ void __launch_bounds__(256) k_overlay_blend(uint8_t* __restrict__ img, const float* __restrict__ mplane, const float* __restrict__ partial,
                                                       int nb, const uint8_t* __restrict__ lut, uint8_t* __restrict__ index, int a256, int h, int w,
                                                       int H, int W) {
    __shared__ float s_lo[256], s_hi[256];
    const int n = blockIdx.y, t = threadIdx.x, total = H * W;
    if (t < nb) {
        s_lo[t] = partial[((size_t)n * nb + t) * 2];
        s_hi[t] = partial[((size_t)n * nb + t) * 2 + 1];
    }
    __syncthreads();
    if (t == 0) {                                     // fixed-order finish of the per-workgroup partials
        float lo = s_lo[0], hi = s_hi[0];
        for (int i = 1; i < nb; ++i) {
            lo = fminf(lo, s_lo[i]);
            hi = fmaxf(hi, s_hi[i]);
        }
        s_lo[0] = lo;
        s_hi[0] = hi;
    }
    __syncthreads();
    const float lo = s_lo[0], den = (s_hi[0] - lo) + 1e-8f;
    const float* m = mplane + (size_t)n * h * w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = blockIdx.x * 1024 + j * 256 + t;
        if (i >= total) break;
        const int y = i / W;
        const float v = __fdiv_rn(ov_resized(m, h, w, H, W, y, i - y * W) - lo, den);
        const float s = floorf(255.f * v);
        const int idx = s >= 0.f ? (s <= 255.f ? (int)s : 255) : 0;      // NaN -> 0
        const size_t at = (size_t)n * total + i;
        if (index) index[at] = (uint8_t)idx;
        uint8_t* p = img + at * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = (uint8_t)(((int)p[c] * (256 - a256) + (int)lut[idx * 3 + c] * a256 + 128) >> 8);
    }
}

extern "C" int pk_heatmap_overlay_ws_floats(int N, int K, int h, int w, int H, int W) {
    if (N <= 0 || K <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t n = (int64_t)N * h * w + (int64_t)N * ov_blocks(H, W) * 2;
    return n > 0x7fffffff ? 0 : (int)n;
}

extern "C" int pk_heatmap_overlay(void* images_u8, const float* heatmaps, float alpha, const void* lut_u8, void* index_u8, float* ws, int N,
                                  int K, int h, int w, int H, int W, void* stream) {
    PK_REQUIRE(images_u8 && heatmaps && lut_u8 && ws, "pk_heatmap_overlay: null pointer");
    PK_REQUIRE(N > 0 && N <= 65535 && K > 0 && h > 0 && w > 0 && H > 0 && W > 0, "pk_heatmap_overlay: bad shape N=%d K=%d h=%d w=%d H=%d W=%d", N,
               K, h, w, H, W);
    PK_REQUIRE(H <= DRAW_MAX_HW && W <= DRAW_MAX_HW && h <= DRAW_MAX_HW && w <= DRAW_MAX_HW, "pk_heatmap_overlay: planes up to %d x %d",
               DRAW_MAX_HW, DRAW_MAX_HW);
    PK_REQUIRE(pk_heatmap_overlay_ws_floats(N, K, h, w, H, W) > 0, "pk_heatmap_overlay: workspace size overflows");
    PK_REQUIRE(alpha == alpha, "pk_heatmap_overlay: alpha is NaN");
    const float a = rintf(256.f * alpha);
    const int a256 = a <= 0.f ? 0 : (a >= 256.f ? 256 : (int)a);
    const int nb = ov_blocks(H, W), hw = h * w;
    float* mplane = ws;
    float* partial = ws + (size_t)N * hw;
    hipLaunchKernelGGL(k_overlay_max, dim3((hw + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, heatmaps, mplane, K, hw);
    hipLaunchKernelGGL(k_overlay_minmax, dim3(nb, N), dim3(256), 0, (hipStream_t)stream, (const float*)mplane, partial, h, w, H, W);
    hipLaunchKernelGGL(k_overlay_blend, dim3((H * W + 1023) / 1024, N), dim3(256), 0, (hipStream_t)stream, (uint8_t*)images_u8,
                       (const float*)mplane, (const float*)partial, nb, (const uint8_t*)lut_u8, (uint8_t*)index_u8, a256, h, w, H, W);
    return pk_launch_status("pk_heatmap_overlay");
}

// ================================================================================================ heatmap overlay, one stack per person
// Top-down use: patch p is the (K,h,w) stack of one person, patch_matrix[p] the 2x3 float64 map from pixels of frame
// patch_image_index[p] to heat-map pixels (the crop matrix with the heat-map size as its output size: heat pixel x is input pixel
// x w_in / w, the decode's convention).  Rule ("Heatmaps where the crop lies"): m_p = max over K; lo_p / hi_p = min / max of
// m_p over its own h x w plane; frame pixel (X, Y) maps to (s, t) = M_p (X, Y, 1) in float64 and is covered by p iff 0 <= s <= w - 1 and
// 0 <= t <= h - 1; there v_p = (bilinear(m_p; s, t) - lo_p) / (hi_p - lo_p + 1e-8) with the tap expression of ov_resized; a covered
// pixel takes v = max over its covering patches (NaN ignored unless every one is NaN), idx = clamp(floor(255 v), 0, 255), NaN -> 0,
// and the integer blend of pk_heatmap_overlay; an uncovered pixel keeps its bytes.  A maximum and a count: no order, no atomics.
__device__ __forceinline__ double ovp_map(const double a, const double b, const double c, const int X, const int Y) {
    return (a * (double)X + b * (double)Y) + c;       // every operation rounds monotonically: over a rectangle the extremes are at its corners
}

// one workgroup per patch: min and max of its own max plane, fixed order (strided partials, then `ov_block_minmax_store`)
__global__ void __launch_bounds__(256) k_overlay_patch_minmax(const float* __restrict__ mplane, float* __restrict__ stats, int hw) {
    const int p = blockIdx.x;
    const float* m = mplane + (size_t)p * hw;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < hw; i += 256) {
        const float v = m[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    ov_block_minmax_store(lo, hi, [&] { return stats + 2 * (size_t)p; });
}

// Gather over the tiles of k_draw_shapes: a workgroup owns a 32 x 8 tile of one frame, finds the frame's patches by binary search in the
// non-decreasing index and walks them 256 at a time, one candidate per thread.  A candidate survives unless the tile lies wholly on one
// side of its heat-map rectangle: s and t are evaluated at the tile's four corner pixels with the expression every pixel uses, and as
// that expression is monotone in X and in Y the test can never drop a patch that covers a pixel of the tile (it needs no inverse matrix,
// so a singular or ill-conditioned matrix costs nothing but the cull; it is also tighter than the bounding box of a rotated crop).
// Survivors go to LDS (ballot compaction as in k_draw_shapes) and every thread folds them into its own pixel in registers; all lanes
// read the same record, a broadcast.  A tile no patch reaches never reads the image.
__global__ void __launch_bounds__(256) k_overlay_patches_blend(uint8_t* __restrict__ img, const float* __restrict__ mplane,
                                                               const float* __restrict__ stats, const int32_t* __restrict__ patch_img,
                                                               const double* __restrict__ patch_matrix, const uint8_t* __restrict__ lut,
                                                               uint8_t* __restrict__ index, uint8_t* __restrict__ cover, int a256, int P,
                                                               int h, int w, int H, int W) {
    __shared__ double s_m[256][6];
    __shared__ float s_lo[256], s_den[256];
    __shared__ int s_p[256];
    __shared__ int s_wcnt[4];
    const int n = blockIdx.z, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int tx0 = blockIdx.x * DRAW_TW, ty0 = blockIdx.y * DRAW_TH;
    const int tx1 = min(tx0 + DRAW_TW - 1, W - 1), ty1 = min(ty0 + DRAW_TH - 1, H - 1);
    const int px = tx0 + (t & (DRAW_TW - 1)), py = ty0 + (t >> 5);
    const bool live = px < W && py < H;
    const size_t at = ((size_t)n * H + (live ? py : 0)) * W + (live ? px : 0);
    const int p_lo = draw_lower_bound(patch_img, P, n), total = draw_lower_bound(patch_img, P, n + 1) - p_lo;
    const double smax = (double)(w - 1), tmax = (double)(h - 1);
    const int hw = h * w;
    float v = NAN;                                    // fmaxf returns the other operand for a NaN: the first covering patch replaces it
    int cnt = 0;
    for (int base = 0; base < total; base += 256) {
        const int cand = base + t;
        bool keep = false;
        double m[6];
        if (cand < total) {
#pragma unroll
            for (int i = 0; i < 6; ++i) m[i] = patch_matrix[(size_t)(p_lo + cand) * 6 + i];
            const double sa = ovp_map(m[0], m[1], m[2], tx0, ty0), sb = ovp_map(m[0], m[1], m[2], tx1, ty0);
            const double sc = ovp_map(m[0], m[1], m[2], tx0, ty1), sd = ovp_map(m[0], m[1], m[2], tx1, ty1);
            const double ta = ovp_map(m[3], m[4], m[5], tx0, ty0), tb = ovp_map(m[3], m[4], m[5], tx1, ty0);
            const double tc = ovp_map(m[3], m[4], m[5], tx0, ty1), td = ovp_map(m[3], m[4], m[5], tx1, ty1);
            const bool out = (sa < 0. && sb < 0. && sc < 0. && sd < 0.) || (sa > smax && sb > smax && sc > smax && sd > smax) ||
                             (ta < 0. && tb < 0. && tc < 0. && td < 0.) || (ta > tmax && tb > tmax && tc > tmax && td > tmax);
            keep = !out;                              // a NaN compares false: kept here, covered nowhere
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wcnt[wv] = __popcll(bal);
        __syncthreads();
        int off = 0, count = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = s_wcnt[i];
            off += i < wv ? c : 0;
            count += c;
        }
        if (keep) {
            const int slot = off + __popcll(bal & ((1ull << lane) - 1ull));      // < 256
#pragma unroll
            for (int i = 0; i < 6; ++i) s_m[slot][i] = m[i];
            const float lo = stats[2 * (size_t)(p_lo + cand)];
            s_lo[slot] = lo;
            s_den[slot] = (stats[2 * (size_t)(p_lo + cand) + 1] - lo) + 1e-8f;
            s_p[slot] = p_lo + cand;
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < count; ++i) {
                const double s = ovp_map(s_m[i][0], s_m[i][1], s_m[i][2], px, py), u = ovp_map(s_m[i][3], s_m[i][4], s_m[i][5], px, py);
                if (!(s >= 0. && s <= smax && u >= 0. && u <= tmax)) continue;
                const int x0 = (int)s, y0 = (int)u;   // floor of a value in [0, n - 1]
                const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
                const float fx = (float)(s - (double)x0), fy = (float)(u - (double)y0);
                const float r = ov_bilinear(mplane + (size_t)s_p[i] * hw, w, y0, y1, x0, x1, fy, fx);
                v = fmaxf(v, __fdiv_rn(r - s_lo[i], s_den[i]));
                ++cnt;
            }
        }
        __syncthreads();                              // the records are rewritten by the next 256 candidates
    }
    if (!live) return;
    int idx = 0;
    if (cnt > 0) {
        const float s = floorf(255.f * v);
        idx = s >= 0.f ? (s <= 255.f ? (int)s : 255) : 0;      // NaN -> 0
        uint8_t* p = img + at * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = (uint8_t)(((int)p[c] * (256 - a256) + (int)lut[idx * 3 + c] * a256 + 128) >> 8);
    }
    if (index) index[at] = (uint8_t)idx;
    if (cover) cover[at] = (uint8_t)min(cnt, 255);
}

extern "C" int pk_heatmap_overlay_patches_ws_floats(int P, int K, int h, int w) {
    if (P <= 0 || K <= 0 || h <= 0 || w <= 0) return 0;
    const int64_t n = (int64_t)P * h * w + (int64_t)P * 2;
    return n > 0x7fffffff ? 0 : (int)n;
}

extern "C" int pk_heatmap_overlay_patches(void* images_u8, const float* heatmaps, const int32_t* patch_image_index, const double* patch_matrix,
                                          float alpha, const void* lut_u8, void* index_u8, void* cover_u8, float* ws, int N, int P, int K, int h,
                                          int w, int H, int W, void* stream) {
    PK_REQUIRE(images_u8 && heatmaps && patch_image_index && patch_matrix && lut_u8 && ws, "pk_heatmap_overlay_patches: null pointer");
    PK_REQUIRE(N > 0 && N <= 65535 && P > 0 && K > 0 && h > 0 && w > 0 && H > 0 && W > 0,
               "pk_heatmap_overlay_patches: bad shape N=%d P=%d K=%d h=%d w=%d H=%d W=%d", N, P, K, h, w, H, W);
    PK_REQUIRE(P <= 65535, "pk_heatmap_overlay_patches: at most 65535 patches in one call (got %d)", P);
    PK_REQUIRE(H <= DRAW_MAX_HW && W <= DRAW_MAX_HW && h <= DRAW_MAX_HW && w <= DRAW_MAX_HW, "pk_heatmap_overlay_patches: planes up to %d x %d",
               DRAW_MAX_HW, DRAW_MAX_HW);
    PK_REQUIRE(pk_heatmap_overlay_patches_ws_floats(P, K, h, w) > 0, "pk_heatmap_overlay_patches: workspace size overflows");
    PK_REQUIRE(alpha == alpha, "pk_heatmap_overlay_patches: alpha is NaN");
    const float a = rintf(256.f * alpha);
    const int a256 = a <= 0.f ? 0 : (a >= 256.f ? 256 : (int)a);
    const int hw = h * w;
    float* mplane = ws;
    float* stats = ws + (size_t)P * hw;
    hipLaunchKernelGGL(k_overlay_max, dim3((hw + 255) / 256, P), dim3(256), 0, (hipStream_t)stream, heatmaps, mplane, K, hw);
    hipLaunchKernelGGL(k_overlay_patch_minmax, dim3(P), dim3(256), 0, (hipStream_t)stream, (const float*)mplane, stats, hw);
    hipLaunchKernelGGL(k_overlay_patches_blend, dim3((W + DRAW_TW - 1) / DRAW_TW, (H + DRAW_TH - 1) / DRAW_TH, N), dim3(256), 0,
                       (hipStream_t)stream, (uint8_t*)images_u8, (const float*)mplane, (const float*)stats, patch_image_index, patch_matrix,
                       (const uint8_t*)lut_u8, (uint8_t*)index_u8, (uint8_t*)cover_u8, a256, P, h, w, H, W);
    return pk_launch_status("pk_heatmap_overlay_patches");
}
