// Feature sheets and heat-map quality (this project's own specification: DESIGN.md "Feature sheets and heat-map quality").  The reference's
// FeatureVisualizer (analysis/nn_quantitative_viz.py:255-324) copies a layer's tensor to the host, normalises every channel with numpy and
// hands the tiles to matplotlib.  Here the tensor stays where it lies:
//   pk_gather_planes     the wanted channels of one sample of an NHWC bf16 map as fp32 planes (16-byte channel groups, kept lanes)
//   pk_plane_sheet       every tile's range, then the whole uint8 sheet: tiles through their colour ramps, everything else background
//   pk_heatmap_quality   one 16-column float64 record per (prediction, target) pair of maps: sums, peaks, co-moments, half-maximum overlap
// No atomics, no last-arriver; every floating-point sum is taken in a fixed order (per thread in ascending index, then `block_reduce`), and
// the colour index is a fixed sequence of fp32 operations (the unit is built without FMA contraction): same input, same bits.
#include "pk_common.h"

#define PNL_THREADS 256                                           // the analysis units' workgroup
#define PNL_WAVES (PNL_THREADS / PK_WAVE)
#define PNL_GRID_CAP 65536                                        // workgroups stride over tiles / maps / pixels beyond this
#define PNL_LIST 8                                                // pk_gather_planes: list entries per thread (one 16-byte load serves a run of them)

// ================================================================================================ channel planes
// Thread (p, q): pixel p of sample b, list entries 8 q .. 8 q + 7.  The 16-byte group of a wanted channel is loaded once for a run of
// entries that fall into it (the first n channels: one load per 8 planes); a channel outside [0, c_used) is never turned into an address.
__global__ void __launch_bounds__(PNL_THREADS) k_gather_planes(const uint4* __restrict__ x, const int32_t* __restrict__ channels,
                                                               float* __restrict__ out, uint32_t HW, uint32_t groups, uint32_t n,
                                                               int32_t c_used, size_t first_pixel) {
    const uint32_t i0 = blockIdx.y * PNL_LIST, i1 = min(i0 + PNL_LIST, n);
    for (uint32_t p = blockIdx.x * PNL_THREADS + threadIdx.x; p < HW; p += gridDim.x * PNL_THREADS) {
        const uint4* __restrict__ px = x + (first_pixel + p) * groups;
        int32_t held = -1;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        for (uint32_t i = i0; i < i1; ++i) {
            const int32_t c = channels[i];
            float f = __uint_as_float(0x7fc00000u);
            if (c >= 0 && c < c_used) {
                if ((c >> 3) != held) held = c >> 3, v = px[held];
                const uint32_t pair = (c & 4) ? ((c & 2) ? v.w : v.z) : ((c & 2) ? v.y : v.x);
                f = bf16_to_f32((uint16_t)((c & 1) ? (pair >> 16) : (pair & 0xffffu)));
            }
            out[(size_t)i * HW + p] = f;
        }
    }
}

extern "C" int pk_gather_planes(const void* x, int B, int H, int W, int C, int b, const int32_t* channels, int n, int c_used, float* out,
                                void* stream) {
    PK_REQUIRE(x && channels && out, "pk_gather_planes: null pointer");
    PK_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && (int64_t)H * W <= PK_PANEL_MAX_PLANE, "pk_gather_planes: bad shape B=%d H=%d W=%d C=%d (H W at most %d)",
               B, H, W, C, PK_PANEL_MAX_PLANE);
    PK_REQUIRE(C % 8 == 0, "pk_gather_planes: C=%d is not a multiple of 8", C);
    PK_REQUIRE(b >= 0 && b < B, "pk_gather_planes: sample %d of %d", b, B);
    PK_REQUIRE(n >= 1 && n <= PK_PANEL_MAX_TILES, "pk_gather_planes: %d planes (1 to %d)", n, PK_PANEL_MAX_TILES);
    PK_REQUIRE(c_used >= 1 && c_used <= C, "pk_gather_planes: c_used=%d (1 to C=%d)", c_used, C);
    PK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)channels & 3) == 0,
               "pk_gather_planes: x must be 16-byte aligned, channels and out 4-byte");
    const uint32_t HW = (uint32_t)((int64_t)H * W);
    const dim3 grid(capped_grid((HW + PNL_THREADS - 1) / PNL_THREADS, PNL_GRID_CAP), (n + PNL_LIST - 1) / PNL_LIST);
    hipLaunchKernelGGL(k_gather_planes, grid, dim3(PNL_THREADS), 0, (hipStream_t)stream, (const uint4*)x, channels, out, HW, (uint32_t)(C / 8),
                       (uint32_t)n, (int32_t)c_used, (size_t)b * HW);
    return pk_launch_status("pk_gather_planes");
}

// ================================================================================================ the sheet
struct SheetGeom { int T, h, w, cols, zoom, pad, SH, SW; };

// The size rule and its refusals, under the caller's name
static inline int sheet_geom(const char* who, int T, int h, int w, int cols, int zoom, int pad, SheetGeom& g) {
    PK_REQUIRE(T >= 1 && T <= PK_PANEL_MAX_TILES, "%s: %d tiles (1 to %d)", who, T, PK_PANEL_MAX_TILES);
    PK_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= PK_PANEL_MAX_PLANE, "%s: bad tile h=%d w=%d (each at least 1, h w at most %d)", who, h, w,
               PK_PANEL_MAX_PLANE);
    PK_REQUIRE(cols >= 1 && cols <= PK_PANEL_MAX_TILES, "%s: cols=%d (1 to %d)", who, cols, PK_PANEL_MAX_TILES);
    PK_REQUIRE(zoom >= 1 && zoom <= PK_PANEL_MAX_ZOOM, "%s: zoom=%d (1 to %d)", who, zoom, PK_PANEL_MAX_ZOOM);
    PK_REQUIRE(pad >= 0 && pad <= PK_PANEL_MAX_PAD, "%s: pad=%d (0 to %d)", who, pad, PK_PANEL_MAX_PAD);
    const int64_t rows = ((int64_t)T + cols - 1) / cols;
    const int64_t SH = pad + rows * ((int64_t)h * zoom + pad), SW = pad + (int64_t)cols * ((int64_t)w * zoom + pad);
    PK_REQUIRE(SH <= PK_PANEL_MAX_SIDE && SW <= PK_PANEL_MAX_SIDE, "%s: the sheet would be %lld x %lld pixels (at most %d per side)", who,
               (long long)SH, (long long)SW, PK_PANEL_MAX_SIDE);
    g = SheetGeom{T, h, w, cols, zoom, pad, (int)SH, (int)SW};
    return PK_OK;
}

extern "C" int pk_plane_sheet_size(int T, int h, int w, int cols, int zoom, int pad, int* SH, int* SW) {
    PK_REQUIRE(SH && SW, "pk_plane_sheet_size: null pointer");
    SheetGeom g;
    if (int rc = sheet_geom("pk_plane_sheet_size", T, h, w, cols, zoom, pad, g)) return rc;
    *SH = g.SH;
    *SW = g.SW;
    return PK_OK;
}

struct SheetTile { const float* a; const float* b; int ramp; };    // a == nullptr: the tile names a plane or a ramp that does not exist

__device__ __forceinline__ SheetTile sheet_tile(const float* __restrict__ a, const float* __restrict__ b, const int32_t* __restrict__ tiles, int t,
                                                int Na, int Nb, int L, int hw) {
    const int ia = tiles[3 * t], ib = tiles[3 * t + 1], ramp = tiles[3 * t + 2];
    SheetTile s{nullptr, nullptr, ramp};
    if (ia < 0 || ia >= Na || ib >= Nb || ramp < 0 || ramp >= L) return s;
    s.a = a + (size_t)ia * hw;
    if (ib >= 0) s.b = b + (size_t)ib * hw;
    return s;
}
__device__ __forceinline__ float sheet_value(const SheetTile& s, int e) { return s.b ? fabsf(s.a[e] - s.b[e]) : s.a[e]; }

// One workgroup per tile: minimum and maximum of its finite values (exact, so the order does not matter), +inf / -inf without one
__global__ void __launch_bounds__(PNL_THREADS) k_sheet_ranges(const float* __restrict__ a, const float* __restrict__ b,
                                                              const int32_t* __restrict__ tiles, float* __restrict__ ranges, int T, int Na, int Nb,
                                                              int L, int hw) {
    __shared__ float red[PNL_WAVES];
    for (int t = blockIdx.x; t < T; t += gridDim.x) {              // uniform over the block
        const SheetTile s = sheet_tile(a, b, tiles, t, Na, Nb, L, hw);
        float lo = INFINITY, hi = -INFINITY;
        if (s.a)
            for (int e = threadIdx.x; e < hw; e += PNL_THREADS) {
                const float v = sheet_value(s, e);
                if (isfinite(v)) lo = fminf(lo, v), hi = fmaxf(hi, v);
            }
        lo = block_reduce<PNL_WAVES>(lo, red, MinOp());
        hi = block_reduce<PNL_WAVES>(hi, red, MaxOp());
        if (threadIdx.x == 0) {
            const float nan = __uint_as_float(0x7fc00000u);
            ranges[2 * t] = s.a ? lo : nan;
            ranges[2 * t + 1] = s.a ? hi : nan;
        }
    }
}

// The three bytes of sheet pixel P = Y SW + X as b0 | b1 << 8 | b2 << 16
__device__ __forceinline__ uint32_t sheet_pixel(const float* __restrict__ a, const float* __restrict__ b, const int32_t* __restrict__ tiles,
                                                const uint8_t* __restrict__ luts, const float* __restrict__ ranges, const SheetGeom g, int Na,
                                                int Nb, int L, uint32_t bg, uint32_t P) {
    const int Y = (int)(P / (uint32_t)g.SW), X = (int)(P - (uint32_t)Y * (uint32_t)g.SW);
    const int th = g.h * g.zoom, tw = g.w * g.zoom;
    const int ty = Y - g.pad, tx = X - g.pad;
    if (ty < 0 || tx < 0) return bg;
    const int r = ty / (th + g.pad), c = tx / (tw + g.pad);
    const int iy = ty - r * (th + g.pad), ix = tx - c * (tw + g.pad);
    const int t = r * g.cols + c;
    if (iy >= th || ix >= tw || t >= g.T) return bg;
    const int hw = g.h * g.w;
    const SheetTile s = sheet_tile(a, b, tiles, t, Na, Nb, L, hw);
    if (!s.a) return bg;
    const float v = sheet_value(s, (iy / g.zoom) * g.w + ix / g.zoom);
    int idx = 0;
    if (isfinite(v)) {
        const float lo = ranges[2 * t], hi = ranges[2 * t + 1];
        const float u = (v - lo) / ((hi - lo) + 1e-8f);
        const float f = floorf(255.0f * u);
        idx = f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);       // a NaN u (inf / inf when v - lo overflows) fails both: 0
    }
    const uint8_t* __restrict__ col = luts + ((size_t)s.ramp * 256 + idx) * 3;
    return (uint32_t)col[0] | ((uint32_t)col[1] << 8) | ((uint32_t)col[2] << 16);
}

// Thread j paints pixels 4 j .. 4 j + 3 of the sheet, taken as one flat array: 12 bytes, three whole dwords.  The last npix % 4 pixels
// are written byte by byte by the thread that owns them.  Every byte of the sheet is written exactly once.
__global__ void __launch_bounds__(PNL_THREADS) k_sheet_paint(const float* __restrict__ a, const float* __restrict__ b,
                                                             const int32_t* __restrict__ tiles, const uint8_t* __restrict__ luts,
                                                             const float* __restrict__ ranges, uint8_t* __restrict__ sheet, const SheetGeom g,
                                                             int Na, int Nb, int L, uint32_t bg) {
    const uint32_t npix = (uint32_t)g.SH * (uint32_t)g.SW, quads = (npix + 3) / 4;
    for (uint32_t j = blockIdx.x * PNL_THREADS + threadIdx.x; j < quads; j += gridDim.x * PNL_THREADS) {
        const uint32_t P = 4 * j;
        if (P + 4 <= npix) {
            const uint32_t c0 = sheet_pixel(a, b, tiles, luts, ranges, g, Na, Nb, L, bg, P);
            const uint32_t c1 = sheet_pixel(a, b, tiles, luts, ranges, g, Na, Nb, L, bg, P + 1);
            const uint32_t c2 = sheet_pixel(a, b, tiles, luts, ranges, g, Na, Nb, L, bg, P + 2);
            const uint32_t c3 = sheet_pixel(a, b, tiles, luts, ranges, g, Na, Nb, L, bg, P + 3);
            uint32_t* __restrict__ o = reinterpret_cast<uint32_t*>(sheet + (size_t)P * 3);
            o[0] = c0 | (c1 << 24);
            o[1] = (c1 >> 8) | (c2 << 16);
            o[2] = (c2 >> 16) | (c3 << 8);
        } else {
            for (uint32_t q = P; q < npix; ++q) {
                const uint32_t c = sheet_pixel(a, b, tiles, luts, ranges, g, Na, Nb, L, bg, q);
                sheet[(size_t)q * 3] = (uint8_t)c;
                sheet[(size_t)q * 3 + 1] = (uint8_t)(c >> 8);
                sheet[(size_t)q * 3 + 2] = (uint8_t)(c >> 16);
            }
        }
    }
}

extern "C" int pk_plane_sheet(const float* a, int Na, const float* b, int Nb, const int32_t* tiles, int T, const void* luts_u8, int L,
                              float* ranges, void* sheet_u8, int h, int w, int cols, int zoom, int pad, int bg0, int bg1, int bg2,
                              void* stream) {
    PK_REQUIRE(a && tiles && luts_u8 && ranges && sheet_u8, "pk_plane_sheet: null pointer");
    SheetGeom g;
    if (int rc = sheet_geom("pk_plane_sheet", T, h, w, cols, zoom, pad, g)) return rc;
    PK_REQUIRE(Na >= 1 && Nb >= 0 && (b || Nb == 0) && L >= 1, "pk_plane_sheet: bad counts Na=%d Nb=%d%s L=%d", Na, Nb, b ? "" : " (b is NULL)", L);
    PK_REQUIRE((unsigned)bg0 <= 255u && (unsigned)bg1 <= 255u && (unsigned)bg2 <= 255u, "pk_plane_sheet: background %d %d %d (bytes)", bg0, bg1, bg2);
    PK_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)tiles | (uintptr_t)ranges | (uintptr_t)sheet_u8) & 3) == 0,
               "pk_plane_sheet: a, b, tiles, ranges and the sheet must be 4-byte aligned");
    hipLaunchKernelGGL(k_sheet_ranges, dim3(capped_grid(T, PNL_GRID_CAP)), dim3(PNL_THREADS), 0, (hipStream_t)stream, a, b, tiles, ranges, T, Na,
                       Nb, L, h * w);
    if (int rc = pk_launch_status("pk_plane_sheet (ranges)")) return rc;
    const int64_t quads = ((int64_t)g.SH * g.SW + 3) / 4;
    const uint32_t bg = (uint32_t)bg0 | ((uint32_t)bg1 << 8) | ((uint32_t)bg2 << 16);
    hipLaunchKernelGGL(k_sheet_paint, dim3(capped_grid((quads + PNL_THREADS - 1) / PNL_THREADS, PNL_GRID_CAP)), dim3(PNL_THREADS), 0,
                       (hipStream_t)stream, a, b, tiles, (const uint8_t*)luts_u8, (const float*)ranges, (uint8_t*)sheet_u8, g, Na, Nb, L, bg);
    return pk_launch_status("pk_plane_sheet (paint)");
}

// ================================================================================================ heat-map quality
// pk_heatmap_summary's key of (value, flat index): larger value first, then smaller index; -0 and +0 are one value.  0 = no candidate.
__device__ __forceinline__ unsigned long long quality_max_key(float v, uint32_t idx) {
    if (v == 0.f) v = 0.f;
    const uint32_t bits = __float_as_uint(v);
    const uint32_t asc = (bits >> 31) ? ~bits : (bits | 0x80000000u);
    return ((unsigned long long)asc << 32) | (unsigned long long)(0xffffffffu - idx);
}

// One workgroup per pair of maps, two passes.  Every sum: thread r adds its elements r, r + 256, ... in ascending order to 0.0 in float64,
// then block_reduce (xor butterfly 32 .. 1 inside the wave, then wave 0 + 1 + 2 + 3).  An element counts iff p and g are both finite.
__global__ void __launch_bounds__(PNL_THREADS) k_heatmap_quality(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 double* __restrict__ records, int64_t M, int hw, int w) {
    __shared__ double red_d[PNL_WAVES];
    __shared__ unsigned long long red_k[PNL_WAVES];
    __shared__ int red_i[PNL_WAVES];
    for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {          // uniform over the block
        const float* __restrict__ P = pred + (size_t)m * hw;
        const float* __restrict__ G = gt + (size_t)m * hw;
        double sp = 0.0, sg = 0.0, sd2 = 0.0, dmax = 0.0;
        float bp = -INFINITY, bg = -INFINITY;
        unsigned long long kp = 0ull, kg = 0ull;
        int left_out = 0;
        for (int i = threadIdx.x; i < hw; i += PNL_THREADS) {
            const float p = P[i], g = G[i];
            if (!(isfinite(p) && isfinite(g))) {
                ++left_out;
                continue;
            }
            const double d = (double)p - (double)g;
            sp += (double)p;
            sg += (double)g;
            sd2 += d * d;
            dmax = fmax(dmax, fabs(d));
            if (p > bp) bp = p, kp = quality_max_key(p, (uint32_t)i);
            if (g > bg) bg = g, kg = quality_max_key(g, (uint32_t)i);
        }
        sp = block_reduce<PNL_WAVES>(sp, red_d, SumOp());
        sg = block_reduce<PNL_WAVES>(sg, red_d, SumOp());
        sd2 = block_reduce<PNL_WAVES>(sd2, red_d, SumOp());
        dmax = block_reduce<PNL_WAVES>(dmax, red_d, MaxOp());
        kp = block_reduce<PNL_WAVES>(kp, red_k, MaxOp());
        kg = block_reduce<PNL_WAVES>(kg, red_k, MaxOp());
        left_out = block_reduce<PNL_WAVES>(left_out, red_i, SumOp());
        const int n = hw - left_out;
        const int ip = kp ? (int)(0xffffffffu - (uint32_t)kp) : 0, ig = kg ? (int)(0xffffffffu - (uint32_t)kg) : 0;
        const float peak_p = kp ? P[ip] : -INFINITY, peak_g = kg ? G[ig] : -INFINITY;
        const double mp = sp / (double)n, mg = sg / (double)n;
        const bool peaks = peak_p > 0.f && peak_g > 0.f;
        const float half_p = 0.5f * peak_p, half_g = 0.5f * peak_g;
        double cpg = 0.0, cpp = 0.0, cgg = 0.0;
        int both = 0, either = 0;
        for (int i = threadIdx.x; i < hw; i += PNL_THREADS) {
            const float p = P[i], g = G[i];
            if (!(isfinite(p) && isfinite(g))) continue;
            const double dp = (double)p - mp, dg = (double)g - mg;
            cpg += dp * dg;
            cpp += dp * dp;
            cgg += dg * dg;
            const bool in_p = peaks && p >= half_p, in_g = peaks && g >= half_g;
            both += in_p && in_g;
            either += in_p || in_g;
        }
        cpg = block_reduce<PNL_WAVES>(cpg, red_d, SumOp());
        cpp = block_reduce<PNL_WAVES>(cpp, red_d, SumOp());
        cgg = block_reduce<PNL_WAVES>(cgg, red_d, SumOp());
        both = block_reduce<PNL_WAVES>(both, red_i, SumOp());
        either = block_reduce<PNL_WAVES>(either, red_i, SumOp());
        if (threadIdx.x == 0) {
            double* o = records + (size_t)m * PK_QUALITY_COLS;
            o[0] = sp, o[1] = sg, o[2] = sd2, o[3] = dmax;
            o[4] = (double)peak_p, o[5] = (double)(ip % w), o[6] = (double)(ip / w);
            o[7] = (double)peak_g, o[8] = (double)(ig % w), o[9] = (double)(ig / w);
            o[10] = cpg, o[11] = cpp, o[12] = cgg;
            o[13] = (double)both, o[14] = (double)either, o[15] = (double)left_out;
        }
    }
}

extern "C" int pk_heatmap_quality(const float* pred, const float* gt, double* records, int64_t M, int h, int w, void* stream) {
    PK_REQUIRE(pred && gt && records, "pk_heatmap_quality: null pointer");
    PK_REQUIRE(M > 0 && h > 0 && w > 0 && (int64_t)h * w <= PK_PANEL_MAX_PLANE, "pk_heatmap_quality: bad shape M=%lld h=%d w=%d (h w at most %d)",
               (long long)M, h, w, PK_PANEL_MAX_PLANE);
    PK_REQUIRE((((uintptr_t)pred | (uintptr_t)gt) & 3) == 0 && ((uintptr_t)records & 7) == 0,
               "pk_heatmap_quality: pred and gt must be 4-byte aligned, records 8-byte");
    hipLaunchKernelGGL(k_heatmap_quality, dim3(capped_grid(M, PNL_GRID_CAP)), dim3(PNL_THREADS), 0, (hipStream_t)stream, pred, gt, records, M, h * w,
                       w);
    return pk_launch_status("pk_heatmap_quality");
}
