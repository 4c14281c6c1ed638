// Target generation (T1, T2).  HBM-bound, fp32, one workgroup per map.
#include "pk_common.h"

// ================================================================================================ T1
// One 256-thread workgroup per (b,k) map. Each thread redoes the (cheap) float64 index arithmetic, then the
// block streams the whole map out with 16-byte stores: every element is written exactly once (zeros or LUT).
__global__ void __launch_bounds__(256) k_gaussian_target(const float* __restrict__ kp, const float* __restrict__ vis,
                                                         const float* __restrict__ lut, float* __restrict__ target,
                                                         float* __restrict__ weight, int Hh, int Wh, double sx, double sy,
                                                         double reach, int pn, int pc) {
    const int map = blockIdx.x;
    float w = vis[map];
    bool draw = !(w < 0.5f);
    int x_lo = 0, y_lo = 0, x_hi = 0, y_hi = 0;
    if (draw) {
        // float32 coordinate / float64 stride, then C truncation toward zero (Python int()).
        const double mx = (double)kp[2 * map] / sx, my = (double)kp[2 * map + 1] / sy;
        const double lim = 1.0e9;
        x_lo = (int)fmin(fmax(mx - reach, -lim), lim);
        y_lo = (int)fmin(fmax(my - reach, -lim), lim);
        x_hi = (int)fmin(fmax(mx + reach + 1.0, -lim), lim);
        y_hi = (int)fmin(fmax(my + reach + 1.0, -lim), lim);
        if (x_lo >= Wh || y_lo >= Hh || x_hi < 0 || y_hi < 0) {
            draw = false;
            w = 0.f;
        }
    }
    if (threadIdx.x == 0) weight[map] = w;
    const int c0 = max(0, x_lo), c1 = min(x_hi, Wh), r0 = max(0, y_lo), r1 = min(y_hi, Hh);
    float* out = target + (size_t)map * Hh * Wh;
    const int n = Hh * Wh;
    if ((Wh & 3) == 0) {
        for (int i = threadIdx.x * 4; i < n; i += blockDim.x * 4) {
            const int y = i / Wh, x = i - y * Wh;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int xx = x + j;
                float val = 0.f;
                if (draw && y >= r0 && y < r1 && xx >= c0 && xx < c1) {
                    const int dx = xx - x_lo - pc, dy = y - y_lo - pc;
                    val = lut[dx * dx + dy * dy];
                }
                v[j] = val;
            }
            *reinterpret_cast<float4*>(out + i) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int y = i / Wh, x = i - y * Wh;
            float val = 0.f;
            if (draw && y >= r0 && y < r1 && x >= c0 && x < c1) {
                const int dx = x - x_lo - pc, dy = y - y_lo - pc;
                val = lut[dx * dx + dy * dy];
            }
            out[i] = val;
        }
    }
}

extern "C" int pk_gaussian_target(const float* keypoints, const float* visible, const float* lut, int lut_len, float* target,
                                  float* weight, int B, int K, int Hh, int Wh, double stride_x, double stride_y,
                                  double reach, int patch_n, int patch_c, void* stream) {
    PK_REQUIRE(keypoints && visible && lut && target && weight, "pk_gaussian_target: null pointer");
    PK_REQUIRE(B > 0 && K > 0 && Hh > 0 && Wh > 0, "pk_gaussian_target: bad shape B=%d K=%d H=%d W=%d", B, K, Hh, Wh);
    PK_REQUIRE(stride_x > 0 && stride_y > 0 && reach > 0, "pk_gaussian_target: bad stride/reach");
    const int far = patch_c > patch_n - 1 - patch_c ? patch_c : patch_n - 1 - patch_c;
    PK_REQUIRE(patch_n > 0 && patch_c >= 0 && patch_c < patch_n && lut_len >= 2 * far * far + 1,
               "pk_gaussian_target: LUT of %d entries too short for a %d-wide patch centred at %d", lut_len, patch_n, patch_c);
    PK_REQUIRE((int)(2 * reach + 1) <= patch_n, "pk_gaussian_target: reach %.2f exceeds the %d-wide patch", reach, patch_n);
    PK_REQUIRE(((uintptr_t)target & 15) == 0, "pk_gaussian_target: target must be 16-byte aligned");
    hipLaunchKernelGGL(k_gaussian_target, dim3(B * K), dim3(256), 0, (hipStream_t)stream, keypoints, visible, lut, target, weight,
                       Hh, Wh, stride_x, stride_y, reach, patch_n, patch_c);
    return pk_launch_status("pk_gaussian_target");
}

// ================================================================================================ T2
__global__ void __launch_bounds__(256) k_dense_target(const float* __restrict__ kp, const float* __restrict__ vis,
                                                      float* __restrict__ hm, float* __restrict__ wts, int Hh, int Wh,
                                                      float scx, float scy, float sigma) {
    const int map = blockIdx.x;
    const float cx = kp[2 * map] * scx, cy = kp[2 * map + 1] * scy;   // float32 multiply, as `scaled_keypoints[:,0] *= scale_w`
    const bool on = vis[map] > 0.f && cx >= 0.f && cx < (float)Wh && cy >= 0.f && cy < (float)Hh;
    if (threadIdx.x == 0) wts[map] = on ? 1.f : 0.f;
    const float denom = 2.f * sigma * sigma;
    float* out = hm + (size_t)map * Hh * Wh;
    for (int i = threadIdx.x; i < Hh * Wh; i += blockDim.x) {
        const int y = i / Wh, x = i - y * Wh;
        float v = 0.f;
        if (on) {
            const float dx = (float)x - cx, dy = (float)y - cy;
            v = fmaxf(0.f, expf(-(dx * dx + dy * dy) / denom));
        }
        out[i] = v;
    }
}

extern "C" int pk_dense_target(const float* keypoints, const float* visible, float* heatmaps, float* weights, int B, int K,
                               int Hh, int Wh, float scale_x, float scale_y, float sigma, void* stream) {
    PK_REQUIRE(keypoints && visible && heatmaps && weights, "pk_dense_target: null pointer");
    PK_REQUIRE(B > 0 && K > 0 && Hh > 0 && Wh > 0 && sigma > 0.f, "pk_dense_target: bad shape");
    hipLaunchKernelGGL(k_dense_target, dim3(B * K), dim3(256), 0, (hipStream_t)stream, keypoints, visible, heatmaps, weights, Hh,
                       Wh, scale_x, scale_y, sigma);
    return pk_launch_status("pk_dense_target");
}
