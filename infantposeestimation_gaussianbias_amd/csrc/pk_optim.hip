// S1: AdamW over ONE flat fp32 parameter buffer (all 11.57 M HRFormer-small parameters = one launch).
// HBM-bound: reads p,g,m,v (16 B/elem) + flag, writes p,m,v (+ bf16 copy): 4 elements per lane, 16-byte accesses.
// Guarded step (opt-in): k_grad_sumsq -> k_grad_guard_finalize -> k_adamw_guarded on one stream.  The global gradient norm and the
// "a gradient is inf/NaN" decision stay on the device; no atomics, every reduction in a fixed order (bit-reproducible, capturable).
#include "pk_common.h"

#define PK_OPTIM_MAX_BLOCKS 2048

static inline int64_t optim_blocks(int64_t n) {
    int64_t blocks = ((n >> 2) + 255) / 256;
    return blocks > PK_OPTIM_MAX_BLOCKS ? PK_OPTIM_MAX_BLOCKS : blocks;
}

// The update of the AdamW kernels: everything after the learning rate, the step number and the gradient factor are known.  The lane's
// first float4 and the grid stride come from the kernel (blockDim read inside a device function compiles to a slower lookup).
// EMA: e += ema_w * (p_new - e) on the elements that were updated, with p_new still in registers (ema_w = 1 - d_t; +8 B/elem).  With
// EMA = false neither `ema` nor `ema_w` is read, and k_adamw / k_adamw_guarded compile to the code they had before the flag existed.
template <bool EMA>
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, const uint8_t* __restrict__ flags, uint16_t* __restrict__ pb,
                                             int64_t n, int64_t first, int64_t stride, float lr, float t, float b1, float b2, float eps,
                                             float wd, float gscale, float* __restrict__ ema, float ema_w) {
    const float bc1 = 1.f - powf(b1, t), bc2s = sqrtf(1.f - powf(b2, t));
    const float step_size = lr / bc1;
    const int64_t n4 = n >> 2;
    for (int64_t i = first; i < n4; i += stride) {
        float4 P = reinterpret_cast<float4*>(p)[i], G = reinterpret_cast<const float4*>(g)[i];
        float4 M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
        const uint32_t f4 = reinterpret_cast<const uint32_t*>(flags)[i];
        float4 E;
        if constexpr (EMA) E = reinterpret_cast<float4*>(ema)[i];
        float* pp = &P.x; float* gg = &G.x; float* mm = &M.x; float* vv = &V.x; float* ee = &E.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t f = (f4 >> (8 * j)) & 0xff;
            if (f & 2u) {  // bit1: parameter takes part in optimisation (receives gradients)
                const float gr = gg[j] * gscale;
                if (f & 1u) pp[j] *= 1.f - lr * wd;  // bit0: decoupled weight decay
                mm[j] = b1 * mm[j] + (1.f - b1) * gr;
                vv[j] = b2 * vv[j] + (1.f - b2) * gr * gr;
                pp[j] -= step_size * mm[j] / (sqrtf(vv[j]) / bc2s + eps);
                if constexpr (EMA) ee[j] = ee[j] + ema_w * (pp[j] - ee[j]);
            }
        }
        reinterpret_cast<float4*>(p)[i] = P;
        reinterpret_cast<float4*>(m)[i] = M;
        reinterpret_cast<float4*>(v)[i] = V;
        if constexpr (EMA) reinterpret_cast<float4*>(ema)[i] = E;  // elements without bit1 go back as they came
        if (pb) {
            uint2 o;
            o.x = pack_bf16x2(P.x, P.y);
            o.y = pack_bf16x2(P.z, P.w);
            reinterpret_cast<uint2*>(pb)[i] = o;
        }
    }
}

__global__ void __launch_bounds__(256) k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, const uint8_t* __restrict__ flags, uint16_t* __restrict__ pb,
                                               int64_t n, const float* __restrict__ lr_dev, const int32_t* __restrict__ step_dev,
                                               float b1, float b2, float eps, float wd, float gscale) {
    adamw_update<false>(p, g, m, v, flags, pb, n, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x,
                        lr_dev[0], (float)step_dev[0], b1, b2, eps, wd, gscale, nullptr, 0.f);
}

// guard_state (written by k_grad_guard_finalize): [0] norm (float), [1] coef (float), [2] skipped_last, [3] skipped_total (int32)
__global__ void __launch_bounds__(256) k_adamw_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, const uint8_t* __restrict__ flags,
                                                       uint16_t* __restrict__ pb, int64_t n, const float* __restrict__ lr_dev,
                                                       const int32_t* __restrict__ step_dev, float b1, float b2, float eps, float wd,
                                                       float gscale, const int32_t* __restrict__ guard_state) {
    if (guard_state[2]) return;  // a gradient was inf/NaN: p, m, v and the bf16 copy keep their values
    const float coef = __int_as_float(guard_state[1]);
    adamw_update<false>(p, g, m, v, flags, pb, n, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x,
                        lr_dev[0], (float)step_dev[0], b1, b2, eps, wd, gscale * coef, nullptr, 0.f);
}

// The update plus the weight average.  guard_state == NULL: k_adamw's update, else k_adamw_guarded's.  The decay is worked out here, in
// every launch, from the same step count as the bias correction (applied updates, >= 1): d_t = min(ema_decay, (1 + t) / (10 + t)), so
// a replayed graph and a guarded run advance the warm-up with no host write, and a skipped step leaves `ema` alone with everything else.
__global__ void __launch_bounds__(256) k_adamw_ema(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, const uint8_t* __restrict__ flags, uint16_t* __restrict__ pb,
                                                   int64_t n, const float* __restrict__ lr_dev, const int32_t* __restrict__ step_dev,
                                                   float b1, float b2, float eps, float wd, float gscale,
                                                   const int32_t* __restrict__ guard_state, float* __restrict__ ema, float ema_decay) {
    if (guard_state) {
        if (guard_state[2]) return;  // a gradient was inf/NaN: p, m, v, the bf16 copy and ema keep their values
        gscale *= __int_as_float(guard_state[1]);
    }
    const float t = (float)step_dev[0];
    const float d = fminf(ema_decay, (1.f + t) / (10.f + t));
    adamw_update<true>(p, g, m, v, flags, pb, n, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x,
                       lr_dev[0], t, b1, b2, eps, wd, gscale, ema, 1.f - d);
}

// Fixed-order sum over the 256 lanes of a workgroup (fp64 has no wave_sum): LDS tree, one barrier per level.  Result in s[0] / bad[0].
__device__ __forceinline__ void block_tree_sum(double* s, uint32_t* bad) {
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s[threadIdx.x] += s[threadIdx.x + w];
            bad[threadIdx.x] |= bad[threadIdx.x + w];
        }
        __syncthreads();
    }
}

// Sum of g^2 over the elements that take part in optimisation (flag bit1), fp64 per lane over the same grid-stride sequence as k_adamw.
// partials[2b] = workgroup b's sum, partials[2b+1] = 1.0 when it saw an element whose exponent bits are all ones (inf / NaN), else 0.0.
__global__ void __launch_bounds__(256) k_grad_sumsq(const float* __restrict__ g, const uint8_t* __restrict__ flags, int64_t n,
                                                    double* __restrict__ partials) {
    __shared__ double s[256];
    __shared__ uint32_t bad[256];
    double acc = 0.0;
    uint32_t nonfinite = 0;
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        const uint32_t f4 = reinterpret_cast<const uint32_t*>(flags)[i];
        const float* gg = &G.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((f4 >> (8 * j)) & 2u) {
                nonfinite |= (__float_as_uint(gg[j]) & 0x7f800000u) == 0x7f800000u;
                const double d = (double)gg[j];
                acc += d * d;  // the square of an fp32 value is exact in fp64
            }
        }
    }
    s[threadIdx.x] = acc;
    bad[threadIdx.x] = nonfinite;
    block_tree_sum(s, bad);
    if (threadIdx.x == 0) {
        double2 o;
        o.x = s[0];
        o.y = bad[0] ? 1.0 : 0.0;
        reinterpret_cast<double2*>(partials)[blockIdx.x] = o;
    }
}

// One workgroup: lane t adds partials t, t+256, ... in that order, then the LDS tree.  norm / clip coefficient / skip decision of the
// step; step_dev counts APPLIED updates (as torch.optim.AdamW under GradScaler, which does not step on a skipped iteration).
__global__ void __launch_bounds__(256) k_grad_guard_finalize(const double* __restrict__ partials, int n_partials, float grad_scale,
                                                             float max_norm, int32_t* __restrict__ guard_state,
                                                             int32_t* __restrict__ step_dev) {
    __shared__ double s[256];
    __shared__ uint32_t bad[256];
    double acc = 0.0;
    uint32_t nonfinite = 0;
    for (int b = threadIdx.x; b < n_partials; b += 256) {
        const double2 pr = reinterpret_cast<const double2*>(partials)[b];
        acc += pr.x;
        nonfinite |= pr.y != 0.0;
    }
    s[threadIdx.x] = acc;
    bad[threadIdx.x] = nonfinite;
    block_tree_sum(s, bad);
    if (threadIdx.x == 0) {
        const double norm = (double)grad_scale * sqrt(s[0]);
        const double mx = (double)max_norm;
        const double c = mx / (norm + 1e-6);  // torch.nn.utils.clip_grad_norm_
        const float coef = (max_norm > 0.f && isfinite(max_norm) && c < 1.0) ? (float)c : 1.0f;
        const int32_t skip = bad[0] ? 1 : 0;
        guard_state[0] = __float_as_int((float)norm);
        guard_state[1] = __float_as_int(coef);
        guard_state[2] = skip;
        guard_state[3] += skip;
        if (!skip) step_dev[0] += 1;
    }
}

static int adamw_check(const char* who, const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                       const uint8_t* decay_mask, const uint16_t* param_bf16, int64_t n, const float* lr_dev, const int32_t* step_dev) {
    PK_REQUIRE(param && grad && exp_avg && exp_avg_sq && decay_mask && lr_dev && step_dev, "%s: null pointer", who);
    PK_REQUIRE(n > 0 && (n & 3) == 0, "%s: n=%lld must be a positive multiple of 4 (pad the flat buffer)", who, (long long)n);
    PK_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0 &&
                   ((uintptr_t)decay_mask & 3) == 0 && ((uintptr_t)param_bf16 & 7) == 0,
               "%s: buffers must be 16-byte aligned", who);
    return PK_OK;
}

extern "C" int pk_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                             uint16_t* param_bf16, int64_t n, const float* lr_dev, const int32_t* step_dev, float beta1,
                             float beta2, float eps, float weight_decay, float grad_scale, void* stream) {
    if (int rc = adamw_check("pk_adamw_step", param, grad, exp_avg, exp_avg_sq, decay_mask, param_bf16, n, lr_dev, step_dev)) return rc;
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)optim_blocks(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                       decay_mask, param_bf16, n, lr_dev, step_dev, beta1, beta2, eps, weight_decay, grad_scale);
    return pk_launch_status("pk_adamw_step");
}

extern "C" int pk_grad_sumsq_partials(int64_t n) {
    PK_REQUIRE(n > 0 && (n & 3) == 0, "pk_grad_sumsq_partials: n=%lld must be a positive multiple of 4", (long long)n);
    return (int)optim_blocks(n);
}

extern "C" int pk_grad_sumsq(const float* grad, const uint8_t* flags, int64_t n, double* partials, int n_partials, void* stream) {
    PK_REQUIRE(grad && flags && partials, "pk_grad_sumsq: null pointer");
    PK_REQUIRE(n > 0 && (n & 3) == 0, "pk_grad_sumsq: n=%lld must be a positive multiple of 4 (pad the flat buffer)", (long long)n);
    PK_REQUIRE(((uintptr_t)grad & 15) == 0 && ((uintptr_t)flags & 3) == 0 && ((uintptr_t)partials & 15) == 0,
               "pk_grad_sumsq: grad / partials must be 16-byte aligned, flags 4-byte aligned");
    PK_REQUIRE(n_partials == (int)optim_blocks(n), "pk_grad_sumsq: n_partials=%d, but n=%lld needs %d (pk_grad_sumsq_partials)",
               n_partials, (long long)n, (int)optim_blocks(n));
    hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)n_partials), dim3(256), 0, (hipStream_t)stream, grad, flags, n, partials);
    return pk_launch_status("pk_grad_sumsq");
}

extern "C" int pk_grad_guard_finalize(const double* partials, int n_partials, float grad_scale, float max_norm, int32_t* guard_state,
                                      int32_t* step_dev, void* stream) {
    PK_REQUIRE(partials && guard_state && step_dev, "pk_grad_guard_finalize: null pointer");
    PK_REQUIRE(n_partials > 0 && n_partials <= PK_OPTIM_MAX_BLOCKS, "pk_grad_guard_finalize: n_partials=%d outside [1, %d]", n_partials,
               PK_OPTIM_MAX_BLOCKS);
    PK_REQUIRE(((uintptr_t)partials & 15) == 0 && ((uintptr_t)guard_state & 3) == 0, "pk_grad_guard_finalize: misaligned buffer");
    hipLaunchKernelGGL(k_grad_guard_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, grad_scale, max_norm,
                       guard_state, step_dev);
    return pk_launch_status("pk_grad_guard_finalize");
}

extern "C" int pk_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                                     uint16_t* param_bf16, int64_t n, const float* lr_dev, const int32_t* step_dev, float beta1,
                                     float beta2, float eps, float weight_decay, float grad_scale, const int32_t* guard_state,
                                     void* stream) {
    if (int rc = adamw_check("pk_adamw_step_guarded", param, grad, exp_avg, exp_avg_sq, decay_mask, param_bf16, n, lr_dev, step_dev))
        return rc;
    PK_REQUIRE(guard_state && ((uintptr_t)guard_state & 3) == 0, "pk_adamw_step_guarded: guard_state is null or misaligned");
    hipLaunchKernelGGL(k_adamw_guarded, dim3((unsigned)optim_blocks(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, decay_mask, param_bf16, n, lr_dev, step_dev, beta1, beta2, eps, weight_decay, grad_scale, guard_state);
    return pk_launch_status("pk_adamw_step_guarded");
}

extern "C" int pk_adamw_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                                 uint16_t* param_bf16, int64_t n, const float* lr_dev, const int32_t* step_dev, float beta1, float beta2,
                                 float eps, float weight_decay, float grad_scale, const int32_t* guard_state, float* ema, float ema_decay,
                                 void* stream) {
    if (int rc = adamw_check("pk_adamw_step_ema", param, grad, exp_avg, exp_avg_sq, decay_mask, param_bf16, n, lr_dev, step_dev)) return rc;
    PK_REQUIRE(ema && ((uintptr_t)ema & 15) == 0, "pk_adamw_step_ema: ema is null or not 16-byte aligned");
    PK_REQUIRE((uintptr_t)ema >= (uintptr_t)(param + n) || (uintptr_t)(ema + n) <= (uintptr_t)param,
               "pk_adamw_step_ema: ema overlaps param (the average needs a buffer of its own)");
    PK_REQUIRE(ema_decay > 0.f && ema_decay < 1.f, "pk_adamw_step_ema: ema_decay=%g must be finite and in (0, 1)",  // false for NaN too
               (double)ema_decay);
    PK_REQUIRE(((uintptr_t)guard_state & 3) == 0, "pk_adamw_step_ema: guard_state is misaligned");
    hipLaunchKernelGGL(k_adamw_ema, dim3((unsigned)optim_blocks(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                       decay_mask, param_bf16, n, lr_dev, step_dev, beta1, beta2, eps, weight_decay, grad_scale, guard_state, ema,
                       ema_decay);
    return pk_launch_status("pk_adamw_step_ema");
}
