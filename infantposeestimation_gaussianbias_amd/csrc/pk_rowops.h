// What the HBM-bound units around the MFMA contractions share (pk_bn.hip BatchNorm, pk_ln.hip LayerNorm and partial sums, pk_exchange.hip
// exchange-unit sum and up-sampling backward, pk_layout.hip layout conversion and packing).  All of them work on NHWC bf16 rows of C
// channels, 8 channels (one 16-byte chunk) per lane.
#pragma once
#include "pk_common.h"

// Workgroups of a grid-stride kernel over `chunks` 16-byte chunks: 256 lanes, `lanes` of them per chunk, at most `cap` workgroups.  The
// kernels that split a chunk index into coordinates do it in 32 bits: with `who` set, 2^32 - 1 chunks or more are refused under that name.
static inline int chunk_grid(size_t chunks, int lanes, size_t cap, const char* who, unsigned& blocks) {
    PK_SUPPORTED(!who || chunks < 0xffffffffull, "%s: tensor too large for 32-bit chunk indices", who);
    const size_t nb = (chunks * lanes + 255) / 256;
    blocks = (unsigned)(nb > cap ? cap : nb);
    return PK_OK;
}
#define CHUNK_GRID_CAP 4096          // one problem per launch
#define CHUNK_GRID_CAP_GROUPED 2048  // per member of a grouped launch

// k_sum_partials (pk_ln.hip): out[k] = scale * sum_b partial[b*stride + k] (+ out[k] with `accumulate`), k < K; out_lo / out_hi: optional
// second copy, split at column `split` into two destinations.  Launch only: the caller reports the launch status under its own name.
#define RED_LANES 64
void sum_partials_launch(const float* partial, int nb, int K, int stride, float* out, float scale, int accumulate, float* out_lo, float* out_hi, int split,
                         hipStream_t stream);

// floor(q / d) for 0 <= q < 2^24: float estimate + one correction (~8 VALU; a 32-bit division by a run-time divisor is ~35)
__device__ __forceinline__ uint32_t fdiv24(uint32_t q, uint32_t d, float inv) {
    int r = (int)((float)q * inv);
    const int rem = (int)q - r * (int)d;
    r += rem >= (int)d ? 1 : (rem < 0 ? -1 : 0);
    return (uint32_t)r;
}
__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    uint4 v;
    v.x = pack_bf16x2(f[0], f[1]);
    v.y = pack_bf16x2(f[2], f[3]);
    v.z = pack_bf16x2(f[4], f[5]);
    v.w = pack_bf16x2(f[6], f[7]);
    return v;
}

// ReLU masks as BITS (round 4): the forward BatchNorm + ReLU kernels can emit one byte per 16-byte chunk (bit j: channel j of the chunk is
// > 0 after the ReLU, taken from the bf16 value that is stored), and the backward kernels read that byte instead of the 16 bytes of the
// activated output: 2 of the 7 tensor passes of a ReLU layer's BatchNorm backward (dy, y, raw read twice; dx written) become 1/16 as large.
__device__ __forceinline__ uint32_t pos_mask8(const uint4& v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = w[i] & 0xffffu, hi = w[i] >> 16;
        m |= ((lo != 0u && !(lo & 0x8000u)) ? 1u : 0u) << (2 * i);
        m |= ((hi != 0u && !(hi & 0x8000u)) ? 1u : 0u) << (2 * i + 1);
    }
    return m;
}
