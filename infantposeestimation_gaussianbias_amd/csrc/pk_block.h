// What the two fused halves of the HRFormer block (pk_block_mlp.hip, pk_block_attn.hip) share: the MFMA shorthands, the bf16 pack /
// unpack helpers, the weight-fragment staging and the per-row LayerNorm.
//
// Everything chains through MFMA accumulator registers (v_mfma_f32_16x16x32_bf16, weight tile = A operand):
//   * a lane of the accumulator tile D[i][j] holds column j = lane & 15 (a token) and rows i = 4g + r, g = lane >> 4 (channels);
//   * two accumulator tiles packed to bf16 ARE the B operand of the next MFMA if its contraction index is enumerated in
//     accumulator order (slot jj of lane group g  <->  row 16 (jj >> 2) + 4 g + (jj & 3) of the stacked tiles).  Hidden units
//     are an internal index, so instead of permuting the second weight matrix the ROWS of W1 (and of b1, W2^T) are gathered in
//     the order that makes accumulator order == natural order: tile t = 2s + u, row i  <->  hidden unit
//     32 s + 8 (i >> 2) + 4 u + (i & 3)   (hid() below).  Every weight fragment is then one contiguous 16-byte read.
//   * weights live in LDS in FRAGMENT ORDER: fragment f is the 1 KiB block [f][lane] of 16-byte pieces, filled once per
//     workgroup, read with lane-linear ds_read_b128 (conflict free by construction, immediate offsets).
//   * LayerNorm statistics: a token's C channels sit in the 4 lanes {j, j+16, j+32, j+48} -> two xor-shuffles.
//   * contractions over TOKENS (weight gradients) need "lane = channel, slots = tokens": activations are written row-major to a
//     wave-private LDS tile and read back with the gfx950 transpose read ds_read_b64_tr_b16 (as pk_attn.hip does for V).
// Waves are independent (one 32-token group per wave and iteration, no workgroup barrier inside the loops); all reductions
// have a fixed order (deterministic, no float atomics).
#pragma once
#include "pk_common.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0)
#define LO4(v) __builtin_shufflevector(v, v, 0, 1, 2, 3)        // the two 16-deep operands inside a 32-deep one
#define HI4(v) __builtin_shufflevector(v, v, 4, 5, 6, 7)
#define LDS_FENCE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")     // this wave's LDS writes are visible to its own reads

// (`used`: hid stays out of the compiler's interprocedural range propagation.  That pass narrows `t` to what the callers of ONE unit
// pass -- t < 2 in the attention kernels, t < 4C / 16 in the MLP kernels -- so the instructions of a kernel changed with its neighbours
// in the unit: four attention kernels came out with other operand orders once the MLP kernels had moved to a unit of their own.)
__attribute__((used)) __device__ __forceinline__ int hid(int t, int i) { return 32 * (t >> 1) + 8 * (i >> 2) + 4 * (t & 1) + (i & 3); }
__device__ __forceinline__ float blo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bhi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ bf16x8 pack2(const f32x4 a, const f32x4 b) {
    const u32x4 v = {pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(b[0], b[1]), pack_bf16x2(b[2], b[3])};
    return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ f32x4 unpack4(const u32x2 v) { return (f32x4){blo(v[0]), bhi(v[0]), blo(v[1]), bhi(v[1])}; }
__device__ __forceinline__ u32x2 pack4(const f32x4 v) { return (u32x2){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])}; }
__device__ __forceinline__ float sum8(const bf16x8 f) {
    const u32x4 v = __builtin_bit_cast(u32x4, f);
    return ((blo(v[0]) + bhi(v[0])) + (blo(v[1]) + bhi(v[1]))) + ((blo(v[2]) + bhi(v[2])) + (blo(v[3]) + bhi(v[3])));
}

// Fragment (column col0 + (lane & 15), k = the tile's 32 rows in ACCUMULATOR order: slots 0..3 = rows 4g .. 4g+3, slots 4..7 =
// rows 16 + 4g .. 16 + 4g + 3) of a row-major [32][pitch] bf16 LDS tile.  EXEC must be all ones (cross-lane gather).
__device__ __forceinline__ bf16x8 tr_frag32(const uint16_t* tile, int pitch, int col0, int lane) {
    const int g = lane >> 4, i = lane & 15;
    const uint16_t* a0 = tile + (4 * g + (i >> 2)) * pitch + col0 + 4 * (i & 3);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 16 * pitch));
    return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// Stage `nfrag` weight fragments into LDS in fragment order: lane (i = l & 15, g = l >> 4) of fragment f receives the 16 bytes
// src[row(f, i)][k0(f) + 8 g .. + 7]  (`ld` = row pitch of src in elements).
template <typename RowFn, typename K0Fn>
__device__ __forceinline__ void stage_frags(u32x4* dst, const uint16_t* __restrict__ src, int nfrag, int ld, RowFn row, K0Fn k0) {
    for (int idx = threadIdx.x; idx < nfrag * 64; idx += blockDim.x) {
        const int f = idx >> 6, l = idx & 63;
        dst[idx] = *reinterpret_cast<const u32x4*>(src + (size_t)row(f, l & 15) * ld + k0(f) + 8 * (l >> 4));
    }
}
#define LDS_FRAG(base, f, lane) __builtin_bit_cast(bf16x8, (base)[(f) * 64 + (lane)])
// The weight fragments in LDS do not change from token group to token group, so LICM would hoist every ds_read out of the group
// loop into registers (C = 64: 64+ fragments = 256+ VGPRs -> occupancy 1 / spills).  An opaque copy of the lane id, made
// inside the loop, keeps the reads where they are; where the hoisted fragments are affordable (forward, C = 32: 64 VGPRs) the
// plain lane id is used and the weights end up register-resident.
template <bool OPAQUE>
__device__ __forceinline__ int opaque_lane(int lane) {
    if (OPAQUE) asm volatile("" : "+v"(lane));
    return lane;
}

// Declares gam / bet for ln_row below: gamma / beta of the channels lane group g holds, 32k + 8g .. + 7 of K-step k.  (A macro: as an
// inline function it changed the instructions of k_mlp_fwd, k_mlp_bwd_dx, k_mlp_bwd_dw<64, 32> and k_attn_fwd<64>.)
#define LN_AFFINE_LOAD(gam, bet, NK, gamma, beta, g)              \
    float gam[NK][8], bet[NK][8];                                 \
    _Pragma("unroll") for (int k_ = 0; k_ < NK; ++k_)             \
        _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) {        \
            gam[k_][j_] = (gamma)[32 * k_ + 8 * (g) + j_];        \
            bet[k_][j_] = (beta)[32 * k_ + 8 * (g) + j_];         \
        }
// LayerNorm of one token row spread over the 4 lanes {j, j+16, j+32, j+48}: lane g holds channels 32k + 8g .. + 7 of K-step k
// (natural order = the B-operand fragment).  Two-pass statistics as k_ln_fwd (pk_ln.hip).
template <int NK>
__device__ __forceinline__ void ln_row(const u32x4 (&xr)[NK], const float (&gam)[NK][8], const float (&bet)[NK][8], float inv_c, float eps,
                                       bf16x8 (&vf)[NK], float& mean, float& rstd) {
    float v[NK][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[k][2 * j] = blo(xr[k][j]);
            v[k][2 * j + 1] = bhi(xr[k][j]);
            s += v[k][2 * j] + v[k][2 * j + 1];
        }
    s = xor16_sum(s);
    s = xor32_sum(s);
    mean = s * inv_c;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[k][j] -= mean;
            q += v[k][j] * v[k][j];
        }
    q = xor16_sum(q);
    q = xor32_sum(q);
    rstd = rsqrtf(q * inv_c + eps);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = pack_bf16x2(v[k][2 * j] * rstd * gam[k][2 * j] + bet[k][2 * j], v[k][2 * j + 1] * rstd * gam[k][2 * j + 1] + bet[k][2 * j + 1]);
        vf[k] = __builtin_bit_cast(bf16x8, o);
    }
}
template <int NK>
__device__ __forceinline__ void scale_rows(const u32x4 (&r)[NK], float sc, bf16x8 (&f)[NK]) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(blo(r[k][j]) * sc, bhi(r[k][j]) * sc);
        f[k] = __builtin_bit_cast(bf16x8, o);
    }
}

// Raise a kernel's dynamic-LDS limit to `bytes` the first time the launcher that expands this is run (the flag is the launcher's: one
// per instantiation); returns the HIP error from the launcher if the runtime refuses.
#define PK_RAISE_LDS_LIMIT_ONCE(who, kernel, bytes)                                                                     \
    do {                                                                                                                \
        static bool raised = false;                                                                                     \
        if (!raised) {                                                                                                  \
            hipError_t e_ = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); \
            if (e_ != hipSuccess) {                                                                                     \
                pk_set_error(who ": cannot raise the LDS limit: %s", hipGetErrorString(e_));                            \
                return (int)e_;                                                                                         \
            }                                                                                                           \
            raised = true;                                                                                              \
        }                                                                                                               \
    } while (0)
