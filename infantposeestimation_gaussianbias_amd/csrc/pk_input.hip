// The input pipeline: affine crop, colour jitter and normalisation, from the decoded uint8 images to the network input.
#include "pk_common.h"

// ================================================================================================ f2: input pipeline
// TopdownAffine(+rotation) image crop + RandomFlip + ToTensor/normalise of the reference's data pipeline (datasets/transforms.py:42-47,
// 128-131, 212-217; datasets/coco_dataset.py:156-163; inference.py:93-110) for a whole batch in ONE launch, straight from the decoded
// uint8 images to the network input.  The warp follows OpenCV's 8-bit `warpAffine(INTER_LINEAR, BORDER_CONSTANT 0)` integer algorithm as
// restated in oracle/warp.py (coordinates in 10-bit fixed point rounded half-to-even, 5 bits of sub-pixel position, weights that sum to
// 2^15, (sum + 2^14) >> 15) -- integer work, bit-exact against that restatement; cv2 itself is not in the image (parity unpinned vs cv2).
// Normalisation is the reference's fp32 expression ((v / 255) - mean) / std with correctly rounded divisions.
struct CropDesc {
    int64_t src_offset;      // byte offset of this sample's (H, W, 3) uint8 image inside the source buffer
    int32_t H, W;
    int32_t flip;            // mirror the source columns (RandomFlip flips the image before the warp)
    int32_t bgr;             // source is BGR (cv2.imread / inference.py:83): swap to RGB
    double minv[6];          // inverse (destination -> source) affine matrix, float64 as OpenCV holds it
};
// The warp of one destination pixel -> its three RGB bytes.  Shared by every crop kernel, so the fused and the jittered path cannot drift.
__device__ __forceinline__ void crop_warp_u8(const unsigned char* __restrict__ src, const CropDesc& d, int x, int y, int u[3]) {
    auto sat = [](double v) { return (long long)max(-2147483648.0, min(2147483647.0, rint(v))); };
    const long long adelta = sat(__dmul_rn(__dmul_rn(d.minv[0], (double)x), 1024.0)), bdelta = sat(__dmul_rn(__dmul_rn(d.minv[3], (double)x), 1024.0));
    const long long X0 = sat(__dmul_rn(__dadd_rn(__dmul_rn(d.minv[1], (double)y), d.minv[2]), 1024.0)) + 16;
    const long long Y0 = sat(__dmul_rn(__dadd_rn(__dmul_rn(d.minv[4], (double)y), d.minv[5]), 1024.0)) + 16;
    const long long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const long long sx = max(-32768LL, min(32767LL, X >> 5)), sy = max(-32768LL, min(32767LL, Y >> 5));
    const int a = (int)(X & 31), b = (int)(Y & 31);
    const int w4[4] = {(32 - a) * (32 - b) * 32, a * (32 - b) * 32, (32 - a) * b * 32, a * b * 32};
    int acc[3] = {0, 0, 0};
    const unsigned char* img = src + d.src_offset;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const long long xx = sx + (t & 1), yy = sy + (t >> 1);
        if (xx < 0 || xx >= d.W || yy < 0 || yy >= d.H) continue;
        const long long xs = d.flip ? d.W - 1 - xx : xx;
        const unsigned char* p = img + (yy * d.W + xs) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += w4[t] * (int)p[d.bgr ? 2 - c : c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = min(255, max(0, (acc[c] + (1 << 14)) >> 15));
}
// ((u / 255) - mean) / std of one pixel's bytes, written as fp32 NCHW and / or bf16 NHWC-8.
__device__ __forceinline__ void crop_normalize_store(const int u[3], int sample, int pix, size_t plane, float* __restrict__ out_nchw,
                                                     uint16_t* __restrict__ out_nhwc8, const float mean[3], const float sd[3]) {
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u[c], 255.0f), mean[c]), sd[c]);
    if (out_nchw) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out_nchw[((size_t)sample * 3 + c) * plane + pix] = v[c];
    }
    if (out_nhwc8) {
        uint4 o;
        o.x = pack_bf16x2(v[0], v[1]);
        o.y = pack_bf16x2(v[2], 0.f);
        o.z = o.w = 0u;
        *reinterpret_cast<uint4*>(out_nhwc8 + ((size_t)sample * plane + pix) * 8) = o;
    }
}
__global__ void __launch_bounds__(256) k_affine_crop(const unsigned char* __restrict__ src, const CropDesc* __restrict__ desc, int out_w, int out_h,
                                                     float* __restrict__ out_nchw, uint16_t* __restrict__ out_nhwc8, float m0, float m1, float m2,
                                                     float s0, float s1, float s2) {
    const CropDesc d = desc[blockIdx.y];
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= out_w * out_h) return;
    const int y = pix / out_w, x = pix - y * out_w;
    int u[3];
    crop_warp_u8(src, d, x, y, u);
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    crop_normalize_store(u, blockIdx.y, pix, (size_t)out_w * out_h, out_nchw, out_nhwc8, mean, sd);
}
// What both crop entries ask of their pointers: a source, a table, at least one output, mean and std; a 16-byte aligned NHWC output if any
static inline bool crop_pointers_ok(const void* src_u8, const void* desc, const void* out_nchw, const void* out_nhwc8, const float* mean3, const float* std3) {
    return src_u8 && desc && (out_nchw || out_nhwc8) && mean3 && std3;
}
static inline bool nhwc8_aligned(const void* out_nhwc8) { return !out_nhwc8 || (((uintptr_t)out_nhwc8) & 15) == 0; }
extern "C" int pk_affine_crop_normalize(const void* src_u8, const void* desc_table, int n_samples, int out_w, int out_h, float* out_nchw_f32,
                                        void* out_nhwc8_bf16, const float* mean3, const float* std3, void* stream) {
    PK_REQUIRE(crop_pointers_ok(src_u8, desc_table, out_nchw_f32, out_nhwc8_bf16, mean3, std3) && n_samples > 0 && out_w > 0 && out_h > 0,
               "pk_affine_crop_normalize: bad argument");
    PK_REQUIRE(nhwc8_aligned(out_nhwc8_bf16), "pk_affine_crop_normalize: 16-byte alignment of the NHWC output");
    hipLaunchKernelGGL(k_affine_crop, dim3((out_w * out_h + 255) / 256, n_samples), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src_u8,
                       (const CropDesc*)desc_table, out_w, out_h, out_nchw_f32, (uint16_t*)out_nhwc8_bf16, mean3[0], mean3[1], mean3[2], std3[0],
                       std3[1], std3[2]);
    return pk_launch_status("pk_affine_crop_normalize");
}

// ------------------------------------------------------------------------------------------------ f2 + colour jitter
// The reference's CustomColorJitter (data/examples.py:367-401) between the 8-bit warp and the normalisation, per sample:
//   x = u8 / 255 * b;   x = (x - m) * c + m, m = mean of x over the crop;   x = g + (x - g) * s, g = mean of the pixel's 3 channels;
//   u8' = trunc(clip(x, 0, 1) * 255)
// m needs the whole crop, so this is two launches: k_crop_u8 warps to a packed-byte scratch and leaves one exact integer sum per
// workgroup; k_jitter_normalize re-adds the sample's partial sums itself (integers: every order gives the same S; no atomics, no
// last-arriver), applies the arithmetic below with one rounding per operation, and normalises like k_affine_crop.  A sample whose
// `enable` is 0 skips the arithmetic altogether: factors (1, 1, 1) are NOT the identity (u8 / 255 * 255 truncates).
struct JitterDesc {
    int32_t enable;
    float b, c, s;           // brightness, contrast, saturation factors
};
__global__ void __launch_bounds__(256) k_crop_u8(const unsigned char* __restrict__ src, const CropDesc* __restrict__ desc, int out_w, int out_h,
                                                 uint32_t* __restrict__ crop, uint32_t* __restrict__ partial) {
    __shared__ uint32_t red[4];
    const CropDesc d = desc[blockIdx.y];
    const int pix = blockIdx.x * 256 + threadIdx.x, plane = out_w * out_h;
    uint32_t sum = 0;                    // a thread past the end of the crop adds nothing
    if (pix < plane) {
        const int y = pix / out_w, x = pix - y * out_w;
        int u[3];
        crop_warp_u8(src, d, x, y, u);
        crop[(size_t)blockIdx.y * plane + pix] = (uint32_t)u[0] | ((uint32_t)u[1] << 8) | ((uint32_t)u[2] << 16);
        sum = (uint32_t)(u[0] + u[1] + u[2]);
    }
    sum = block_reduce<4>(sum, red, SumOp());          // exact, unsigned
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}
__global__ void __launch_bounds__(256) k_jitter_normalize(const uint32_t* __restrict__ crop, const uint32_t* __restrict__ partial,
                                                          const JitterDesc* __restrict__ jit, int out_w, int out_h, float* __restrict__ out_nchw,
                                                          uint16_t* __restrict__ out_nhwc8, float m0, float m1, float m2, float s0, float s1,
                                                          float s2) {
    __shared__ uint32_t red[4];
    const JitterDesc j = jit[blockIdx.y];
    const int pix = blockIdx.x * 256 + threadIdx.x, plane = out_w * out_h;
    float m = 0.f;
    if (j.enable) {                      // uniform over the block
        uint32_t S = 0;                  // < 2^32: the entry point rejects crops with 765 h w >= 2^32
        for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) S += partial[(size_t)blockIdx.y * gridDim.x + i];
        S = block_reduce<4>(S, red, SumOp());
        m = (float)__dmul_rn(__ddiv_rn((double)S, __dmul_rn(255.0, (double)plane * 3.0)), (double)j.b);
    }
    if (pix >= plane) return;
    const uint32_t p = crop[(size_t)blockIdx.y * plane + pix];
    int u[3] = {(int)(p & 255u), (int)((p >> 8) & 255u), (int)(p >> 16)};
    if (j.enable) {
        float x[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = __fmul_rn(__fdiv_rn((float)u[c], 255.0f), j.b);
            x[c] = __fadd_rn(__fmul_rn(__fsub_rn(x[c], m), j.c), m);
        }
        const float g = __fdiv_rn(__fadd_rn(__fadd_rn(x[0], x[1]), x[2]), 3.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = fminf(fmaxf(__fadd_rn(g, __fmul_rn(__fsub_rn(x[c], g), j.s)), 0.f), 1.f);
            u[c] = (int)__fmul_rn(v, 255.0f);
        }
    }
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    crop_normalize_store(u, blockIdx.y, pix, (size_t)plane, out_nchw, out_nhwc8, mean, sd);
}
// Workspace: n * w * h packed crop pixels, then n * ceil(w h / 256) partial sums, all uint32.  PK_ERR_INVALID (and an error string) if the
// shape is refused.
static inline int64_t jitter_partial_offset(int n_samples, int out_w, int out_h) { return (int64_t)n_samples * out_w * out_h; }   // in uint32 words
extern "C" int pk_affine_crop_jitter_ws_bytes(int n_samples, int out_w, int out_h) {
    PK_REQUIRE(n_samples > 0 && out_w > 0 && out_h > 0 && (int64_t)out_w * out_h * 765 < (int64_t)1 << 32,
               "pk_affine_crop_jitter_ws_bytes: bad shape n=%d w=%d h=%d (the byte sum of a crop must stay below 2^32)", n_samples, out_w, out_h);
    const int64_t nblk = ((int64_t)out_w * out_h + 255) / 256, bytes = 4 * (jitter_partial_offset(n_samples, out_w, out_h) + n_samples * nblk);
    PK_REQUIRE(bytes <= 0x7fffffff, "pk_affine_crop_jitter_ws_bytes: %lld-byte workspace for n=%d w=%d h=%d exceeds 2^31", (long long)bytes,
               n_samples, out_w, out_h);
    return (int)bytes;
}
extern "C" int pk_affine_crop_jitter_normalize(const void* src_u8, const void* desc_table, const void* jitter_table, int n_samples, int out_w,
                                               int out_h, float* out_nchw_f32, void* out_nhwc8_bf16, const float* mean3, const float* std3,
                                               void* ws, int64_t ws_bytes, void* stream) {
    PK_REQUIRE(crop_pointers_ok(src_u8, desc_table, out_nchw_f32, out_nhwc8_bf16, mean3, std3) && jitter_table && ws,
               "pk_affine_crop_jitter_normalize: null pointer");
    const int need = pk_affine_crop_jitter_ws_bytes(n_samples, out_w, out_h);       // the shape checks live there
    if (need < 0) return need;
    PK_REQUIRE(ws_bytes >= need, "pk_affine_crop_jitter_normalize: workspace of %lld bytes, %d needed", (long long)ws_bytes, need);
    PK_REQUIRE((((uintptr_t)ws) & 3) == 0 && nhwc8_aligned(out_nhwc8_bf16),
               "pk_affine_crop_jitter_normalize: alignment (workspace 4 bytes, NHWC output 16 bytes)");
    const int nblk = (out_w * out_h + 255) / 256;
    uint32_t* crop = (uint32_t*)ws;
    uint32_t* partial = crop + jitter_partial_offset(n_samples, out_w, out_h);
    hipLaunchKernelGGL(k_crop_u8, dim3(nblk, n_samples), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src_u8, (const CropDesc*)desc_table,
                       out_w, out_h, crop, partial);
    hipLaunchKernelGGL(k_jitter_normalize, dim3(nblk, n_samples), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)crop, (const uint32_t*)partial,
                       (const JitterDesc*)jitter_table, out_w, out_h, out_nchw_f32, (uint16_t*)out_nhwc8_bf16, mean3[0], mean3[1], mean3[2],
                       std3[0], std3[1], std3[2]);
    return pk_launch_status("pk_affine_crop_jitter_normalize");
}

// ------------------------------------------------------------------------------------------------ f2 + occlusion, blur, noise
// This project's own augmentation of the warped bytes (DESIGN.md "Occlusion, blur and noise on the device"; the contract is in
// posekernels.h): colour jitter, separable integer Gaussian blur, hashed sensor noise and rectangle erasing between the 8-bit warp and the
// normalisation.  Launch 1 is k_crop_u8 as above; k_augment_normalize then takes one 32 x 32 output tile of one sample per workgroup.
// With the blur on it loads the tile and an R-pixel halo (clamped coordinates, jittered on the way in), runs the horizontal pass from one
// LDS image into a second and the vertical pass into registers; with the blur off it touches no LDS beyond the reduction of S.
struct AugRect {
    int32_t x0, y0, x1, y1;
    int32_t mode;            // 0: the constant `rgb`, otherwise hashed bytes
    uint32_t rgb;            // r | g << 8 | b << 16
};
struct AugDesc {
    JitterDesc jit;
    int32_t radius;
    int32_t q[PK_AUG_MAX_RADIUS + 1];
    int32_t amp;
    uint32_t noise_seed;
    int32_t n_rects;
    uint32_t erase_seed;
    AugRect rect[PK_AUG_MAX_RECTS];
    int32_t pad[3];
};
static_assert(sizeof(AugDesc) == PK_AUG_ROW_BYTES && PK_AUG_ROW_BYTES % 16 == 0, "aug_table row layout");
// The jitter arithmetic of k_jitter_normalize on one pixel's bytes, m given.
__device__ __forceinline__ void jitter_pixel_u8(int u[3], float b, float c, float s, float m) {
    float x[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        x[ch] = __fmul_rn(__fdiv_rn((float)u[ch], 255.0f), b);
        x[ch] = __fadd_rn(__fmul_rn(__fsub_rn(x[ch], m), c), m);
    }
    const float g = __fdiv_rn(__fadd_rn(__fadd_rn(x[0], x[1]), x[2]), 3.0f);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float v = fminf(fmaxf(__fadd_rn(g, __fmul_rn(__fsub_rn(x[ch], g), s)), 0.f), 1.f);
        u[ch] = (int)__fmul_rn(v, 255.0f);
    }
}
__device__ __forceinline__ uint32_t aug_hash(uint32_t seed, uint32_t pix, uint32_t stream) {
    uint32_t x = seed + pix * 0x9E3779B9u + stream * 0x85EBCA6Bu;
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
// One blur tap on a packed pixel: red and blue share a register as two 16-bit fields.  A field's sum is at most 255 * 256 + 128 = 65408,
// so it never carries into its neighbour.
__device__ __forceinline__ void blur_tap(uint32_t p, uint32_t q, uint32_t& rb, uint32_t& g) {
    rb += (p & 0x00FF00FFu) * q;
    g += ((p >> 8) & 0xFFu) * q;
}
__device__ __forceinline__ uint32_t blur_round(uint32_t rb, uint32_t g) {
    return (((rb + 0x00800080u) >> 8) & 0x00FF00FFu) | (((g + 128u) >> 8) << 8);
}
constexpr int kAugTile = 32, kAugSpan = kAugTile + 2 * PK_AUG_MAX_RADIUS;
__global__ void __launch_bounds__(256) k_augment_normalize(const uint32_t* __restrict__ crop, const uint32_t* __restrict__ partial,
                                                           const AugDesc* __restrict__ aug, int out_w, int out_h, float* __restrict__ out_nchw,
                                                           uint16_t* __restrict__ out_nhwc8, float m0, float m1, float m2, float s0, float s1,
                                                           float s2) {
    // A half-wave is 32 consecutive columns of one row in every pass, so each 4-byte LDS access of a 32-lane group covers 32 consecutive
    // dwords = 32 different banks, whatever the row stride: neither the horizontal nor the vertical pass serialises.
    __shared__ uint32_t red[4];
    __shared__ uint32_t ta[kAugSpan * kAugSpan];         // jittered tile + halo
    __shared__ uint32_t tb[kAugSpan * kAugTile];         // after the horizontal pass
    __shared__ uint32_t qs[2 * PK_AUG_MAX_RADIUS + 1];   // the taps, -R .. R
    const AugDesc* __restrict__ a = aug + blockIdx.y;    // per-sample fields are uniform over the workgroup
    const int tid = threadIdx.x, plane = out_w * out_h, tiles_x = (out_w + kAugTile - 1) / kAugTile;
    const int ty0 = (int)blockIdx.x / tiles_x, x0 = ((int)blockIdx.x - ty0 * tiles_x) * kAugTile, y0 = ty0 * kAugTile;
    const uint32_t* __restrict__ cs = crop + (size_t)blockIdx.y * plane;
    const int jit_on = a->jit.enable;
    const float jb = a->jit.b, jc = a->jit.c, js = a->jit.s;
    float m = 0.f;
    if (jit_on) {                        // as k_jitter_normalize: the exact S from the partial sums of k_crop_u8
        const int nblk = (plane + 255) / 256;
        uint32_t S = 0;
        for (int i = tid; i < nblk; i += 256) S += partial[(size_t)blockIdx.y * nblk + i];
        S = block_reduce<4>(S, red, SumOp());
        m = (float)__dmul_rn(__ddiv_rn((double)S, __dmul_rn(255.0, (double)plane * 3.0)), (double)jb);
    }
    auto load = [&](int x, int y) -> uint32_t {          // one warped pixel, jittered
        const uint32_t p = cs[y * out_w + x];
        if (!jit_on) return p;
        int u[3] = {(int)(p & 255u), (int)((p >> 8) & 255u), (int)(p >> 16)};
        jitter_pixel_u8(u, jb, jc, js, m);
        return (uint32_t)u[0] | ((uint32_t)u[1] << 8) | ((uint32_t)u[2] << 16);
    };
    const int R = min(max(a->radius, 0), PK_AUG_MAX_RADIUS);
    if (R > 0) {
        const int span = kAugTile + 2 * R;
        if (tid <= 2 * R) qs[tid] = (uint32_t)a->q[abs(tid - R)];
        for (int i = tid; i < span * span; i += 256) {
            const int ly = i / span, lx = i - ly * span;
            ta[ly * kAugSpan + lx] = load(min(max(x0 + lx - R, 0), out_w - 1), min(max(y0 + ly - R, 0), out_h - 1));
        }
        __syncthreads();
        for (int i = tid; i < span * kAugTile; i += 256) {
            const int ly = i / kAugTile, lx = i - ly * kAugTile;
            uint32_t rb = 0, g = 0;
            for (int k = 0; k <= 2 * R; ++k) blur_tap(ta[ly * kAugSpan + lx + k], qs[k], rb, g);
            tb[i] = blur_round(rb, g);
        }
        __syncthreads();
    }
    const int amp = min(max(a->amp, 0), 255), n_rects = min(max(a->n_rects, 0), PK_AUG_MAX_RECTS);
    const uint32_t noise_seed = a->noise_seed, erase_seed = a->erase_seed;
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    const int lx = tid & (kAugTile - 1), x = x0 + lx;
    if (x >= out_w) return;
    for (int ly = tid / kAugTile; ly < kAugTile; ly += 256 / kAugTile) {
        const int y = y0 + ly;
        if (y >= out_h) break;
        uint32_t p;
        if (R > 0) {
            uint32_t rb = 0, g = 0;
            for (int k = 0; k <= 2 * R; ++k) blur_tap(tb[(ly + k) * kAugTile + lx], qs[k], rb, g);
            p = blur_round(rb, g);
        } else {
            p = load(x, y);
        }
        const uint32_t pix = (uint32_t)(y * out_w + x);
        int u[3] = {(int)(p & 255u), (int)((p >> 8) & 255u), (int)(p >> 16)};
        if (amp > 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t h = aug_hash(noise_seed, pix, 0x100u + c);
                const int s = (int)((h & 255u) + ((h >> 8) & 255u) + ((h >> 16) & 255u) + (h >> 24)) - 510;
                u[c] = min(max(u[c] + ((amp * s + 256) >> 9), 0), 255);
            }
        }
        for (int r = 0; r < n_rects; ++r) {
            const AugRect& k = a->rect[r];
            if (x < k.x0 || x >= k.x1 || y < k.y0 || y >= k.y1) continue;
            const uint32_t f = k.mode == 0 ? k.rgb : aug_hash(erase_seed, pix, 1u + r);
            u[0] = (int)(f & 255u), u[1] = (int)((f >> 8) & 255u), u[2] = (int)((f >> 16) & 255u);
        }
        crop_normalize_store(u, blockIdx.y, (int)pix, (size_t)plane, out_nchw, out_nhwc8, mean, sd);
    }
}
extern "C" int pk_affine_crop_augment_ws_bytes(int n_samples, int out_w, int out_h) {
    PK_REQUIRE(n_samples > 0 && out_w > 0 && out_h > 0 && (int64_t)out_w * out_h * 765 < (int64_t)1 << 32,
               "pk_affine_crop_augment_ws_bytes: bad shape n=%d w=%d h=%d (the byte sum of a crop must stay below 2^32)", n_samples, out_w, out_h);
    const int64_t nblk = ((int64_t)out_w * out_h + 255) / 256, bytes = 4 * (jitter_partial_offset(n_samples, out_w, out_h) + n_samples * nblk);
    PK_REQUIRE(bytes <= 0x7fffffff, "pk_affine_crop_augment_ws_bytes: %lld-byte workspace for n=%d w=%d h=%d exceeds 2^31", (long long)bytes,
               n_samples, out_w, out_h);
    return (int)bytes;
}
extern "C" int pk_affine_crop_augment_normalize(const void* src_u8, const void* desc_table, const void* aug_table, int n_samples, int out_w,
                                                int out_h, float* out_nchw_f32, void* out_nhwc8_bf16, const float* mean3, const float* std3,
                                                void* ws, int64_t ws_bytes, void* stream) {
    PK_REQUIRE(crop_pointers_ok(src_u8, desc_table, out_nchw_f32, out_nhwc8_bf16, mean3, std3) && aug_table && ws,
               "pk_affine_crop_augment_normalize: null pointer");
    const int need = pk_affine_crop_augment_ws_bytes(n_samples, out_w, out_h);      // the shape checks live there
    if (need < 0) return need;
    PK_REQUIRE(ws_bytes >= need, "pk_affine_crop_augment_normalize: workspace of %lld bytes, %d needed", (long long)ws_bytes, need);
    PK_REQUIRE((((uintptr_t)ws) & 3) == 0 && nhwc8_aligned(out_nhwc8_bf16) && (((uintptr_t)aug_table) & 15) == 0,
               "pk_affine_crop_augment_normalize: alignment (workspace 4 bytes, NHWC output 16 bytes, augmentation table 16 bytes)");
    const int nblk = (out_w * out_h + 255) / 256;
    const int tiles = ((out_w + kAugTile - 1) / kAugTile) * ((out_h + kAugTile - 1) / kAugTile);
    uint32_t* crop = (uint32_t*)ws;
    uint32_t* partial = crop + jitter_partial_offset(n_samples, out_w, out_h);
    hipLaunchKernelGGL(k_crop_u8, dim3(nblk, n_samples), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src_u8, (const CropDesc*)desc_table,
                       out_w, out_h, crop, partial);
    hipLaunchKernelGGL(k_augment_normalize, dim3(tiles, n_samples), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)crop,
                       (const uint32_t*)partial, (const AugDesc*)aug_table, out_w, out_h, out_nchw_f32, (uint16_t*)out_nhwc8_bf16, mean3[0],
                       mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    return pk_launch_status("pk_affine_crop_augment_normalize");
}
