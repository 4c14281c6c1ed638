// Gradient attribution (this project's own specification: DESIGN.md "Gradient attribution").  The reference computes input saliency
// (SensitivityAnalyzer.compute_input_sensitivity, analysis/advanced_analysis.py:317-342) and Grad-CAM (GradCAMVisualizer.generate_cam,
// analysis/nn_quantitative_viz.py:358-415) with one batch-1 forward / backward per joint and reduces on the host.  Here the maps of all
// joints come from one batched backward, and what autograd cannot do with the packed layouts is four kernels:
//   pk_stem_dgrad             data gradient of the stem's 3x3 stride-2 conv down to the 8-channel packed pixel (a bandwidth kernel)
//   pk_nhwc_bf16_to_nchw_f32  backward of the input pack: packed bf16 gradient -> (B,C,H,W) fp32, exact
//   pk_saliency_reduce        packed gradient -> max over the real channels of |g|, exact, NaN shows
//   pk_gradcam                the reference's four Grad-CAM lines per sample, in float64: a weights launch and a map launch
// No atomics; every reduction in a fixed order (per thread ascending, then `block_reduce`): the same input gives the same bits.
#include "pk_rowops.h"

#define ATT_THREADS 256                                           // the analysis units' workgroup
#define ATT_WAVES (ATT_THREADS / PK_WAVE)
#define ATT_TAPS 9

// ================================================================================================ stem data gradient
// One input pixel per thread and pass.  The forward pack [Cout][9][8] bf16 is staged once per workgroup in LDS as it lies in memory: at a
// given n the threads of a wave read at most nine different addresses (their current tap), 16 bytes apart inside one 144-byte row, i.e.
// on different banks; equal addresses are one broadcast.  CH = 4 reads 8 bytes per tap (c_real <= 4: the RGB stem), CH = 8 reads 16.
// Order of the fp32 sum of channel c: taps ky * 3 + kx ascending, inside a tap n ascending; products of two bf16 values are exact in
// fp32, so the only roundings are those of the additions and the final one to bf16.
template <int CH>
__global__ void __launch_bounds__(ATT_THREADS) k_stem_dgrad(const uint16_t* __restrict__ g, const uint16_t* __restrict__ w, uint4* __restrict__ dx,
                                                            uint32_t pixels, uint32_t Hs, uint32_t Ws, uint32_t Ho, uint32_t Wo, uint32_t Cout,
                                                            uint32_t c_real) {
    extern __shared__ __align__(16) uint16_t lds_w[];             // [Cout][9][8]
    const uint32_t chunks = Cout * ATT_TAPS;                      // 16-byte chunks of the pack
    for (uint32_t i = threadIdx.x; i < chunks; i += ATT_THREADS)
        reinterpret_cast<uint4*>(lds_w)[i] = reinterpret_cast<const uint4*>(w)[i];
    __syncthreads();
    const uint32_t HW = Hs * Ws;
    for (uint32_t i = blockIdx.x * ATT_THREADS + threadIdx.x; i < pixels; i += gridDim.x * ATT_THREADS) {
        const uint32_t b = i / HW, r = i - b * HW;
        const uint32_t y = r / Ws, x = r - y * Ws;
        float acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = 0.f;
        for (uint32_t ky = 0; ky < 3; ++ky) {
            const uint32_t ty = y + 1 - ky;                       // y + 1 >= ky: no wrap
            if ((ty & 1u) || (ty >> 1) >= Ho) continue;
            for (uint32_t kx = 0; kx < 3; ++kx) {
                const uint32_t tx = x + 1 - kx;
                if ((tx & 1u) || (tx >> 1) >= Wo) continue;
                const uint16_t* __restrict__ gp = g + ((size_t)(b * Ho + (ty >> 1)) * Wo + (tx >> 1)) * Cout;
                const uint16_t* wt = lds_w + (ky * 3 + kx) * 8;
                for (uint32_t n0 = 0; n0 < Cout; n0 += 8) {
                    float gv[8];
                    unpack8(*reinterpret_cast<const uint4*>(gp + n0), gv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint16_t* wn = wt + (size_t)(n0 + j) * (ATT_TAPS * 8);
                        if (CH == 4) {
                            const uint2 q = *reinterpret_cast<const uint2*>(wn);
                            acc[0] += gv[j] * __uint_as_float(q.x << 16);
                            acc[1] += gv[j] * __uint_as_float(q.x & 0xffff0000u);
                            acc[2] += gv[j] * __uint_as_float(q.y << 16);
                            acc[3] += gv[j] * __uint_as_float(q.y & 0xffff0000u);
                        } else {
                            float wv[8];
                            unpack8(*reinterpret_cast<const uint4*>(wn), wv);
#pragma unroll
                            for (int c = 0; c < CH; ++c) acc[c] += gv[j] * wv[c];
                        }
                    }
                }
            }
        }
        float out[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) out[c] = 0.f;                 // channels >= c_real: exactly 0, whatever the pack holds there
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if ((uint32_t)c < c_real) out[c] = acc[c];
        dx[i] = pack8(out);
    }
}

extern "C" int pk_stem_dgrad(const void* g, const void* w, void* dx, int B, int Hs, int Ws, int Ho, int Wo, int Cout, int c_real, void* stream) {
    PK_REQUIRE(g && w && dx, "pk_stem_dgrad: null pointer");
    PK_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "pk_stem_dgrad: bad shape B=%d Hs=%d Ws=%d Ho=%d Wo=%d", B, Hs, Ws, Ho, Wo);
    PK_REQUIRE(Cout > 0 && Cout % 8 == 0 && Cout <= PK_STEM_DGRAD_MAX_COUT, "pk_stem_dgrad: Cout=%d (a multiple of 8 up to %d: the weight pack is held in LDS)",
               Cout, PK_STEM_DGRAD_MAX_COUT);
    PK_REQUIRE(c_real >= 1 && c_real <= 8, "pk_stem_dgrad: c_real=%d (1 to 8: the real channels of the 8-channel packed pixel)", c_real);
    PK_REQUIRE(Ho == (Hs - 1) / 2 + 1 && Wo == (Ws - 1) / 2 + 1,
               "pk_stem_dgrad: output %d x %d is not that of a 3x3 stride-2 pad-1 conv of %d x %d (Ho = (Hs - 1) / 2 + 1, Wo likewise)", Ho, Wo, Hs, Ws);
    PK_REQUIRE((int64_t)B * Hs * Ws <= 0x7fffffffll, "pk_stem_dgrad: %d images of %d x %d pixels overflow 32-bit pixel indices", B, Hs, Ws);
    PK_REQUIRE((((uintptr_t)g | (uintptr_t)w | (uintptr_t)dx) & 15) == 0, "pk_stem_dgrad: pointers must be 16-byte aligned");
    const uint32_t pixels = (uint32_t)((int64_t)B * Hs * Ws);
    unsigned gb;
    if (int rc = chunk_grid(pixels, 1, CHUNK_GRID_CAP, "pk_stem_dgrad", gb)) return rc;
    const size_t lds = (size_t)Cout * ATT_TAPS * 8 * sizeof(uint16_t);
    auto kern = c_real <= 4 ? k_stem_dgrad<4> : k_stem_dgrad<8>;
    hipLaunchKernelGGL(kern, dim3(gb), dim3(ATT_THREADS), lds, (hipStream_t)stream, (const uint16_t*)g, (const uint16_t*)w, (uint4*)dx, pixels,
                       (uint32_t)Hs, (uint32_t)Ws, (uint32_t)Ho, (uint32_t)Wo, (uint32_t)Cout, (uint32_t)c_real);
    return pk_launch_status("pk_stem_dgrad");
}

// ================================================================================================ backward of the input pack
// One pixel per thread and pass: the first ceil(C / 8) chunks of its Cpad channels are read, channel c goes to plane c.  bf16 widens exactly.
__global__ void __launch_bounds__(ATT_THREADS) k_nhwc_to_nchw(const uint16_t* __restrict__ g, float* __restrict__ out, uint32_t pixels, uint32_t HW,
                                                              uint32_t C, uint32_t Cp) {
    for (uint32_t i = blockIdx.x * ATT_THREADS + threadIdx.x; i < pixels; i += gridDim.x * ATT_THREADS) {
        const uint32_t b = i / HW, r = i - b * HW;
        float* __restrict__ o = out + (size_t)b * C * HW + r;
        for (uint32_t c0 = 0; c0 < C; c0 += 8) {
            float v[8];
            unpack8(*reinterpret_cast<const uint4*>(g + (size_t)i * Cp + c0), v);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < C) o[(size_t)(c0 + j) * HW] = v[j];
        }
    }
}

extern "C" int pk_nhwc_bf16_to_nchw_f32(const void* g, float* out, int B, int C, int H, int W, int Cpad, void* stream) {
    PK_REQUIRE(g && out, "pk_nhwc_bf16_to_nchw_f32: null pointer");
    PK_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Cpad >= C && (Cpad & 7) == 0,
               "pk_nhwc_bf16_to_nchw_f32: bad argument B=%d C=%d H=%d W=%d Cpad=%d (C <= Cpad, Cpad a multiple of 8)", B, C, H, W, Cpad);
    PK_REQUIRE((int64_t)B * H * W <= 0x7fffffffll, "pk_nhwc_bf16_to_nchw_f32: %d images of %d x %d pixels overflow 32-bit pixel indices", B, H, W);
    PK_REQUIRE(((uintptr_t)g & 15) == 0, "pk_nhwc_bf16_to_nchw_f32: the packed tensor must be 16-byte aligned");
    const uint32_t pixels = (uint32_t)((int64_t)B * H * W);
    unsigned gb;
    if (int rc = chunk_grid(pixels, 1, CHUNK_GRID_CAP, "pk_nhwc_bf16_to_nchw_f32", gb)) return rc;
    hipLaunchKernelGGL(k_nhwc_to_nchw, dim3(gb), dim3(ATT_THREADS), 0, (hipStream_t)stream, (const uint16_t*)g, out, pixels, (uint32_t)(H * W),
                       (uint32_t)C, (uint32_t)Cpad);
    return pk_launch_status("pk_nhwc_bf16_to_nchw_f32");
}

// ================================================================================================ saliency
// max over c < c_real of |g_c|, one 16-byte pixel per thread and pass.  A NaN replaces the running maximum and is never replaced
// (NaN > m and m' > NaN are both false), so a NaN in any real channel gives NaN, as torch.max does; pad channels are not looked at.
__global__ void __launch_bounds__(ATT_THREADS) k_saliency_reduce(const uint4* __restrict__ g, float* __restrict__ out, uint32_t pixels, uint32_t c_real) {
    for (uint32_t i = blockIdx.x * ATT_THREADS + threadIdx.x; i < pixels; i += gridDim.x * ATT_THREADS) {
        float v[8];
        unpack8(g[i], v);
        float m = fabsf(v[0]);
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            const float a = fabsf(v[c]);
            if ((uint32_t)c < c_real && (a > m || a != a)) m = a;
        }
        out[i] = m;
    }
}

extern "C" int pk_saliency_reduce(const void* g, float* out, int B, int H, int W, int c_real, void* stream) {
    PK_REQUIRE(g && out, "pk_saliency_reduce: null pointer");
    PK_REQUIRE(B > 0 && H > 0 && W > 0, "pk_saliency_reduce: bad shape B=%d H=%d W=%d", B, H, W);
    PK_REQUIRE(c_real >= 1 && c_real <= 8, "pk_saliency_reduce: c_real=%d (1 to 8: the real channels of the 8-channel packed pixel)", c_real);
    PK_REQUIRE((int64_t)B * H * W <= 0x7fffffffll, "pk_saliency_reduce: %d images of %d x %d pixels overflow 32-bit pixel indices", B, H, W);
    PK_REQUIRE(((uintptr_t)g & 15) == 0, "pk_saliency_reduce: the packed gradient must be 16-byte aligned");
    const uint32_t pixels = (uint32_t)((int64_t)B * H * W);
    unsigned gb;
    if (int rc = chunk_grid(pixels, 1, CHUNK_GRID_CAP, "pk_saliency_reduce", gb)) return rc;
    hipLaunchKernelGGL(k_saliency_reduce, dim3(gb), dim3(ATT_THREADS), 0, (hipStream_t)stream, (const uint4*)g, out, pixels, (uint32_t)c_real);
    return pk_launch_status("pk_saliency_reduce");
}

// ================================================================================================ Grad-CAM
// Two launches, everything in float64 (DESIGN.md "Gradient attribution" says why two):
//   weights  one workgroup per (sample, 8-channel chunk): thread t adds pixels t, t + 256, ... of its 8 channels in ascending order to 0.0,
//            then `block_reduce` per channel; weight = sum / (h w).  Stored as float64 in the workspace and rounded to fp32 for the caller.
//   map      one workgroup per sample: raw[p] = max(0, sum over c < c_used ascending of weight[c] * A[p][c]) for pixels t, t + 256, ...
//            into the workspace, minimum and maximum by `block_reduce`, then out[p] = (raw[p] - min) / ((max - min) + 1e-8) rounded once.
// A NaN: max(0, NaN) stays NaN here, and a NaN in any raw value makes minimum and maximum NaN, so the whole sample's map is NaN.
// Workspace per sample: Cw = 8 ceil(c_used / 8) weights, then h w raw values.
__global__ void __launch_bounds__(ATT_THREADS) k_gradcam_weights(const uint16_t* __restrict__ G, double* __restrict__ ws, float* __restrict__ weights,
                                                                 uint32_t hw, uint32_t C, uint32_t c_used, uint32_t Cw) {
    __shared__ double red[ATT_WAVES];
    const uint32_t b = blockIdx.y, c0 = blockIdx.x * 8;
    const uint16_t* __restrict__ base = G + (size_t)b * hw * C + c0;
    double s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.0;
    for (uint32_t p = threadIdx.x; p < hw; p += ATT_THREADS) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(base + (size_t)p * C), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += (double)v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double t = block_reduce<ATT_WAVES>(s[j], red, SumOp()) / (double)hw;
        if (threadIdx.x == 0) {
            ws[(size_t)b * (Cw + hw) + c0 + j] = t;
            if (c0 + j < c_used) weights[(size_t)b * c_used + c0 + j] = (float)t;
        }
    }
}

__global__ void __launch_bounds__(ATT_THREADS) k_gradcam_map(const uint16_t* __restrict__ A, double* __restrict__ ws, float* __restrict__ cam,
                                                             double* __restrict__ range, uint32_t hw, uint32_t C, uint32_t c_used, uint32_t Cw) {
    __shared__ double red[ATT_WAVES];
    __shared__ int red_i[ATT_WAVES];
    const uint32_t b = blockIdx.x;
    const double* __restrict__ wt = ws + (size_t)b * (Cw + hw);   // written by the launch before this one
    double* __restrict__ raw = ws + (size_t)b * (Cw + hw) + Cw;
    const uint16_t* __restrict__ a = A + (size_t)b * hw * C;
    double lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (uint32_t p = threadIdx.x; p < hw; p += ATT_THREADS) {
        double s = 0.0;
        for (uint32_t c0 = 0; c0 < c_used; c0 += 8) {
            float v[8];
            unpack8(*reinterpret_cast<const uint4*>(a + (size_t)p * C + c0), v);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < c_used) s += wt[c0 + j] * (double)v[j];
        }
        const double r = (s > 0.0 || s != s) ? s : 0.0;
        raw[p] = r;
        bad |= (r != r);
        lo = r < lo ? r : lo;
        hi = r > hi ? r : hi;
    }
    lo = block_reduce<ATT_WAVES>(lo, red, MinOp());
    hi = block_reduce<ATT_WAVES>(hi, red, MaxOp());
    bad = block_reduce<ATT_WAVES>(bad, red_i, MaxOp());
    if (bad) lo = hi = (double)NAN;
    if (threadIdx.x == 0) range[2 * b] = lo, range[2 * b + 1] = hi;
    const double den = (hi - lo) + 1e-8;
    for (uint32_t p = threadIdx.x; p < hw; p += ATT_THREADS) cam[(size_t)b * hw + p] = (float)((raw[p] - lo) / den);   // the thread's own raw values
}

// float64 workspace of pk_gradcam, counted in 4-byte floats: per sample 8 ceil(c_used / 8) weights and h w raw values
static inline int64_t gradcam_ws_floats(int64_t B, int64_t hw, int64_t c_used) { return 2 * B * ((c_used + 7) / 8 * 8 + hw); }

extern "C" int pk_gradcam_ws_floats(int B, int h, int w, int c_used) {
    if (B <= 0 || h <= 0 || w <= 0 || c_used <= 0) return 0;
    const int64_t hw = (int64_t)h * w;
    PK_REQUIRE(hw <= 0x7fffffffll / 4 && gradcam_ws_floats(B, hw, c_used) <= 0x7fffffffll, "pk_gradcam_ws_floats: B=%d h=%d w=%d c_used=%d is too large", B, h,
               w, c_used);
    return (int)gradcam_ws_floats(B, hw, c_used);
}

extern "C" int pk_gradcam(const void* A, const void* G, double* ws, float* cam, float* weights, double* range, int B, int h, int w, int C, int c_used,
                          void* stream) {
    PK_REQUIRE(A && G && ws && cam && weights && range, "pk_gradcam: null pointer");
    PK_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0, "pk_gradcam: bad shape B=%d h=%d w=%d (B up to 65535: a grid dimension)", B, h, w);
    PK_REQUIRE(C > 0 && C % 8 == 0, "pk_gradcam: C=%d (a multiple of 8: the op layer's 16-byte channel chunks)", C);
    PK_REQUIRE(c_used >= 1 && c_used <= C, "pk_gradcam: c_used=%d (1 to C=%d)", c_used, C);
    const int64_t hw = (int64_t)h * w;
    PK_REQUIRE(hw <= 0x7fffffffll / 4 && gradcam_ws_floats(B, hw, c_used) <= 0x7fffffffll, "pk_gradcam: B=%d h=%d w=%d c_used=%d is too large", B, h, w, c_used);
    PK_REQUIRE((((uintptr_t)A | (uintptr_t)G) & 15) == 0 && ((uintptr_t)ws & 7) == 0, "pk_gradcam: A and G must be 16-byte aligned, the workspace 8-byte");
    const uint32_t Cw = (uint32_t)((c_used + 7) / 8 * 8);
    hipLaunchKernelGGL(k_gradcam_weights, dim3(Cw / 8, B), dim3(ATT_THREADS), 0, (hipStream_t)stream, (const uint16_t*)G, ws, weights, (uint32_t)hw,
                       (uint32_t)C, (uint32_t)c_used, Cw);
    if (int rc = pk_launch_status("pk_gradcam (weights)")) return rc;
    hipLaunchKernelGGL(k_gradcam_map, dim3(B), dim3(ATT_THREADS), 0, (hipStream_t)stream, (const uint16_t*)A, ws, cam, range, (uint32_t)hw, (uint32_t)C,
                       (uint32_t)c_used, Cw);
    return pk_launch_status("pk_gradcam (map)");
}
