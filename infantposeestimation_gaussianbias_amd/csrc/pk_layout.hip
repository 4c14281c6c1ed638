// Input layout conversion, weight packing, the padded-twin box copy, window partition / reverse (pk_rows_by_map) and DropPath.
#include "pk_rowops.h"

// ================================================================================================ layout / packing
// (B,3,H,W) fp32 NCHW -> (B,H,W,Cp) bf16 NHWC with channels >= Cin zero-filled (Cp = 8: 16-byte pixels for the stem)
__global__ void __launch_bounds__(256) k_nchw_to_nhwc(const float* __restrict__ x, uint16_t* __restrict__ y, int B, int Cin, int H, int W,
                                                      int Cp, const float* __restrict__ sp_y) {
    const size_t pixels = (size_t)B * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / ((size_t)H * W), r = i - b * H * W;
        for (int c0 = 0; c0 < Cp; c0 += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float t = 0.f;
                if (c0 + j < Cin) {
                    const size_t k = (b * Cin + c0 + j) * H * W + r;
                    t = x[k];
                    if (sp_y) t *= 1.f - __expf(-sp_y[k]);     // d softplus(z)/dz = sigmoid(z) = 1 - exp(-softplus(z))
                }
                v[j] = t;
            }
            *reinterpret_cast<uint4*>(y + i * Cp + c0) = pack8(v);
        }
    }
}
extern "C" int pk_nchw_f32_to_nhwc_bf16(const float* x, const float* softplus_out, void* y, int B, int Cin, int H, int W, int Cpad,
                                        void* stream) {
    PK_REQUIRE(x && y && B > 0 && Cin > 0 && H > 0 && W > 0 && Cpad >= Cin && (Cpad & 7) == 0, "pk_nchw_f32_to_nhwc_bf16: bad argument");
    const size_t pixels = (size_t)B * H * W;
    unsigned gb;
    chunk_grid(pixels, 1, CHUNK_GRID_CAP, nullptr, gb);          // one lane per pixel, 64-bit indices in the kernel: nothing to refuse
    hipLaunchKernelGGL(k_nchw_to_nhwc, dim3(gb), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)y, B, Cin, H, W, Cpad, softplus_out);
    return pk_launch_status("pk_nchw_f32_to_nhwc_bf16");
}

// Weight packing fp32 -> bf16 compute copies, table driven (ONE launch for the whole model).
//   mode 0: dst[n][t][cp]      = src[n][c][t]            conv forward   (OIHW -> [N][T][Cin_pad])
//   mode 1: dst[c][T-1-t][n]   = src[n][c][t]            conv data-grad (flipped taps, channels swapped), rows padded to Np
//   mode 2: dst[c][n]          = src[n][c]               linear data-grad (transpose)
//   (linear forward is mode 0 with T = 1)
struct PackDesc { const float* src; int64_t dst_off; int N, C, T, mode, Cp, Np; int64_t dst_numel; };
__global__ void __launch_bounds__(256) k_pack_weights(uint16_t* __restrict__ dst, const PackDesc* __restrict__ desc,
                                                      const int* __restrict__ blk_desc, const int* __restrict__ blk_first) {
    const PackDesc d = desc[blk_desc[blockIdx.x]];
    const float* __restrict__ src = d.src;
    const int64_t i0 = (int64_t)(blockIdx.x - blk_first[blockIdx.x]) * 1024;
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k * 256 + threadIdx.x;
        if (i >= d.dst_numel) return;
        float v = 0.f;
        if (d.mode == 0) {
            const int c = (int)(i % d.Cp), t = (int)((i / d.Cp) % d.T), n = (int)(i / ((int64_t)d.Cp * d.T));
            if (c < d.C) v = src[((int64_t)n * d.C + c) * d.T + t];
        } else if (d.mode == 1) {
            const int n = (int)(i % d.Np), t = (int)((i / d.Np) % d.T), c = (int)(i / ((int64_t)d.Np * d.T));
            if (n < d.N) v = src[((int64_t)n * d.C + c) * d.T + (d.T - 1 - t)];
        } else {
            const int n = (int)(i % d.Np), c = (int)(i / d.Np);
            if (n < d.N) v = src[(int64_t)n * d.C + c];
        }
        dst[d.dst_off + i] = f32_to_bf16(v);
    }
}
extern "C" int pk_pack_weights(void* flat_dst_bf16, const void* desc_table, const int32_t* block_desc, const int32_t* block_first,
                               int n_blocks, void* stream) {
    PK_REQUIRE(flat_dst_bf16 && desc_table && block_desc && block_first && n_blocks > 0, "pk_pack_weights: bad argument");
    hipLaunchKernelGGL(k_pack_weights, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, (uint16_t*)flat_dst_bf16,
                       (const PackDesc*)desc_table, block_desc, block_first);
    return pk_launch_status("pk_pack_weights");
}

// ================================================================================================ padded twins
// A model whose channel counts are not multiples of 8 (HRFormer-base: C = 78/156/312/624, head_dim 39) runs through a
// "padded twin" with 8-aligned shapes.  Every real tensor is a box r[0..3] embedded at the origin of the twin's box p[0..3]
// (plain zero-extension, or head-structured: qkv rows (3, heads, 39 -> 40, C -> Cp), proj columns (C -> Cp, heads, 39 -> 40)).
// direction 0: twin[box] = real (parameters / buffers before a forward); 1: real = twin[box] (gradients into a gradient
// sink, BatchNorm running statistics after a step); 2: real += twin[box] (autograd-style accumulation into `.grad`).
// Table driven: ONE launch per direction for the whole model.
struct EmbedDesc { float* real; int64_t twin_off; int r[4]; int p[4]; int64_t numel; };
__global__ void __launch_bounds__(256) k_embed_boxes(float* __restrict__ twin, const EmbedDesc* __restrict__ desc,
                                                     const int* __restrict__ blk_desc, const int* __restrict__ blk_first, int direction) {
    const EmbedDesc d = desc[blk_desc[blockIdx.x]];
    const int64_t i0 = (int64_t)(blockIdx.x - blk_first[blockIdx.x]) * 1024;
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k * 256 + threadIdx.x;
        if (i >= d.numel) return;
        int64_t t = i;
        const int i3 = (int)(t % d.r[3]);
        t /= d.r[3];
        const int i2 = (int)(t % d.r[2]);
        t /= d.r[2];
        const int i1 = (int)(t % d.r[1]), i0_ = (int)(t / d.r[1]);
        const int64_t j = d.twin_off + (((int64_t)i0_ * d.p[1] + i1) * d.p[2] + i2) * d.p[3] + i3;
        if (direction == 0) twin[j] = d.real[i];
        else if (direction == 1) d.real[i] = twin[j];
        else d.real[i] += twin[j];
    }
}
extern "C" int pk_embed_boxes(float* twin_base, const void* desc_table, const int* block_desc, const int* block_first, int n_blocks,
                              int direction, void* stream) {
    PK_REQUIRE(twin_base && desc_table && block_desc && block_first && n_blocks > 0 && direction >= 0 && direction <= 2,
               "pk_embed_boxes: bad argument");
    hipLaunchKernelGGL(k_embed_boxes, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, twin_base, (const EmbedDesc*)desc_table, block_desc,
                       block_first, direction);
    return pk_launch_status("pk_embed_boxes");
}

// window_partition / window_reverse (hrformer.py:67-114) as row moves through the window row map (window-order token -> pixel row, -1 = one
// of the zero tokens appended at the bottom / right): gather = partition (pad tokens read as zeros), scatter = reverse (pad tokens dropped).
// Rows are `row_dwords` 4-byte words of any element type.
__global__ void k_rows_by_map(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const int* __restrict__ map, long n_rows,
                              int row_dwords, int scatter) {
    const long total = n_rows * row_dwords;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / row_dwords;
        const int c = (int)(i - r * row_dwords), pr = map[r];
        if (scatter) {
            if (pr >= 0) dst[(long)pr * row_dwords + c] = src[i];
        } else {
            dst[i] = pr >= 0 ? src[(long)pr * row_dwords + c] : 0u;
        }
    }
}
extern "C" int pk_rows_by_map(const void* src, void* dst, const int* rowmap, int64_t n_rows, int row_bytes, int scatter, void* stream) {
    PK_REQUIRE(src && dst && rowmap && n_rows > 0 && row_bytes > 0 && row_bytes % 4 == 0, "pk_rows_by_map: bad argument (rows of whole dwords)");
    const long total = n_rows * (row_bytes / 4);
    const int nb = capped_grid((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_rows_by_map, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src, (uint32_t*)dst, rowmap, (long)n_rows,
                       row_bytes / 4, scatter);
    return pk_launch_status("pk_rows_by_map");
}

// drop_path (hrformer.py:15-24): out = (x / keep) * mask[sample], mask in {0, 1}; fp32 elements, `per_sample` of them per sample.
__global__ void k_drop_path(const float* __restrict__ x, const float* __restrict__ mask, float* __restrict__ out, long total, long per_sample,
                            float keep) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        out[i] = (x[i] / keep) * mask[i / per_sample];
}
extern "C" int pk_drop_path_f32(const float* x, const float* mask, float* out, int64_t batch, int64_t per_sample, float keep_prob, void* stream) {
    PK_REQUIRE(x && mask && out && batch > 0 && per_sample > 0 && keep_prob > 0.f, "pk_drop_path_f32: bad argument");
    const long total = batch * per_sample;
    const int nb = capped_grid((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_drop_path, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, mask, out, total, (long)per_sample, keep_prob);
    return pk_launch_status("pk_drop_path_f32");
}
