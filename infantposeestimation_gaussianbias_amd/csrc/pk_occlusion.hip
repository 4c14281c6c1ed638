// Occlusion sensitivity (this project's own specification: DESIGN.md "Occlusion sensitivity").  The reference's
// SensitivityAnalyzer.occlusion_sensitivity (analysis/advanced_analysis.py:387-427) clones the image on the host, blanks one patch, runs a
// batch-1 forward and reads one sum back, once per patch position and for one joint.  Here the sweep is a few batched forwards between
// three kernels, with no host round trip, and gives every joint at once:
//   pk_occlude_batch     the occluded copies of one packed image, straight in the stem's layout (bf16 NHWC, 8-channel pixels)
//   pk_heatmap_summary   one 256-thread workgroup per output map: sum, maximum and its position in one pass
//   pk_occlusion_paint   the reference's map from the score table, in gather form (the last writer of its loops, found in closed form)
// No atomics; the one floating-point sum is taken in a fixed order (per thread in ascending index, then `block_reduce`): same bits each run.
#include "pk_rowops.h"

#define OCC_THREADS 256                                           // the analysis units' workgroup
#define OCC_WAVES (OCC_THREADS / PK_WAVE)
#define OCC_MAP_GRID_CAP 65536                                    // pk_heatmap_summary: workgroups stride over the maps beyond this

// ================================================================================================ the grid of patch positions
// Positions along one axis are range(0, extent - patch, stride): ceil((extent - patch) / stride) of them when extent > patch, else none.
// The position extent - patch itself is not taken: the reference's rule, kept.
static inline int64_t occ_positions(int extent, int patch, int stride) {
    return extent > patch ? ((int64_t)extent - patch + stride - 1) / stride : 0;
}

extern "C" int pk_occlusion_positions(int extent, int patch, int stride) {
    PK_REQUIRE(extent >= 1 && patch >= 1 && stride >= 1, "pk_occlusion_positions: bad argument extent=%d patch=%d stride=%d (each at least 1)",
               extent, patch, stride);
    return (int)occ_positions(extent, patch, stride);
}

// ny, nx of an (H, W) image; refuses bad arguments and the empty grid under the caller's name
static inline int occ_grid(const char* who, int H, int W, int patch, int stride, int& ny, int& nx) {
    PK_REQUIRE(H >= 1 && W >= 1 && patch >= 1 && stride >= 1, "%s: bad argument H=%d W=%d patch=%d stride=%d (each at least 1)", who, H, W, patch,
               stride);
    ny = (int)occ_positions(H, patch, stride);
    nx = (int)occ_positions(W, patch, stride);
    PK_REQUIRE(ny > 0 && nx > 0,
               "%s: no patch position: rows and columns start at range(0, extent - patch, stride), which is empty for H=%d W=%d patch=%d", who,
               H, W, patch);
    PK_REQUIRE((int64_t)ny * nx <= 0x7fffffff, "%s: %lld x %lld patch positions", who, (long long)ny, (long long)nx);
    return PK_OK;
}

// ================================================================================================ occluded copies
// fp32 -> bf16 on the host, round to nearest even: the conversion pk_nchw_f32_to_nhwc_bf16 applies on the device
static inline uint32_t host_bf16(float f) {
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (b >> 16) | 0x40u;
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}

// One 16-byte pixel per thread and pass.  Copy c of the launch is position p = first + c = a nx + b; its pixel (y, x) is the image's,
// except inside rows a stride .. a stride + patch - 1 and columns b stride .. b stride + patch - 1, where it is `fill`.
__global__ void __launch_bounds__(OCC_THREADS) k_occlude_batch(const uint4* __restrict__ x, uint4* __restrict__ out, uint32_t HW, uint32_t W,
                                                               uint32_t nx, uint32_t patch, uint32_t stride, uint32_t first, uint64_t total,
                                                               uint4 fill) {
    for (uint64_t i = (uint64_t)blockIdx.x * OCC_THREADS + threadIdx.x; i < total; i += (uint64_t)gridDim.x * OCC_THREADS) {
        const uint32_t j = (uint32_t)i;                           // total < 2^32 - 1 (checked by the entry)
        const uint32_t c = j / HW, r = j - c * HW;
        const uint32_t y = r / W, col = r - y * W;
        const uint32_t p = first + c, a = p / nx, b = p - a * nx;
        const uint32_t dy = y - a * stride, dx = col - b * stride;      // unsigned: a pixel above or left of the patch wraps to a huge value
        uint4 v = x[r];
        if (dy < patch && dx < patch) v = fill;
        out[i] = v;
    }
}

extern "C" int pk_occlude_batch(const void* x, void* out, int H, int W, int patch, int stride, int first, int n, const float* fill_host,
                                void* stream) {
    PK_REQUIRE(x && out, "pk_occlude_batch: null pointer");
    int ny, nx;
    if (int rc = occ_grid("pk_occlude_batch", H, W, patch, stride, ny, nx)) return rc;
    PK_REQUIRE(first >= 0 && n >= 1 && (int64_t)first + n <= (int64_t)ny * nx, "pk_occlude_batch: copies %d .. %lld of %lld (%d x %d positions)",
               first, (long long)first + n - 1, (long long)ny * nx, ny, nx);
    PK_REQUIRE((int64_t)H * W < 0xffffffffll / n, "pk_occlude_batch: %d copies of %d x %d pixels overflow 32-bit pixel indices", n, H, W);
    const size_t total = (size_t)n * H * W;
    const uintptr_t s0 = (uintptr_t)x, s1 = s0 + (size_t)H * W * 16, d0 = (uintptr_t)out, d1 = d0 + total * 16;
    PK_REQUIRE(s1 <= d0 || d1 <= s0, "pk_occlude_batch: the source image lies inside the destination");
    PK_REQUIRE(((s0 | d0) & 15) == 0, "pk_occlude_batch: pointers must be 16-byte aligned");
    unsigned gb;
    if (int rc = chunk_grid(total, 1, CHUNK_GRID_CAP, "pk_occlude_batch", gb)) return rc;
    uint4 fill = make_uint4(0u, 0u, 0u, 0u);                      // the default: 0 in normalised space; pad channels 3..7 always 0
    if (fill_host) {
        fill.x = host_bf16(fill_host[0]) | (host_bf16(fill_host[1]) << 16);
        fill.y = host_bf16(fill_host[2]);
    }
    hipLaunchKernelGGL(k_occlude_batch, dim3(gb), dim3(OCC_THREADS), 0, (hipStream_t)stream, (const uint4*)x, (uint4*)out, (uint32_t)((int64_t)H * W),
                       (uint32_t)W, (uint32_t)nx, (uint32_t)patch, (uint32_t)stride, (uint32_t)first, (uint64_t)total, fill);
    return pk_launch_status("pk_occlude_batch");
}

// ================================================================================================ one summary per map
// Key of (value, flat index) whose unsigned order is: larger value first, then smaller index; -0 and +0 are one value.  0 = no candidate.
__device__ __forceinline__ uint64_t occ_max_key(float v, uint32_t idx) {
    if (v == 0.f) v = 0.f;
    const uint32_t b = __float_as_uint(v);
    const uint32_t asc = (b >> 31) ? ~b : (b | 0x80000000u);
    return ((uint64_t)asc << 32) | (uint64_t)(0xffffffffu - idx);
}

// Map m: thread t adds elements t, t + 256, ... in ascending order to 0.0 in double, then block_reduce (xor butterfly 32 .. 1 inside the
// wave, then wave 0 + 1 + 2 + 3).  Maximum: the thread's candidate starts at -inf with no index and is replaced iff v > best in float, so a
// NaN never wins and among equal values the first index stays; the block takes the largest value, among equals the smallest index.  A
// map without a value above -inf reports max = -inf at index 0.  The stored maximum is the element at the winning index, bit for bit.
__global__ void __launch_bounds__(OCC_THREADS) k_heatmap_summary(const float* __restrict__ heatmaps, double* __restrict__ out, int64_t M, int hw,
                                                                 int w) {
    __shared__ double red_d[OCC_WAVES];
    __shared__ unsigned long long red_k[OCC_WAVES];
    for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {         // uniform over the block
        const float* __restrict__ map = heatmaps + (size_t)m * hw;
        double sum = 0.0;
        float best = -INFINITY;
        unsigned long long key = 0ull;
        for (int i = threadIdx.x; i < hw; i += OCC_THREADS) {
            const float v = map[i];
            sum += (double)v;
            if (v > best) best = v, key = occ_max_key(v, (uint32_t)i);
        }
        const double total = block_reduce<OCC_WAVES>(sum, red_d, SumOp());
        const unsigned long long top = block_reduce<OCC_WAVES>(key, red_k, MaxOp());
        if (threadIdx.x == 0) {
            const int idx = top ? (int)(0xffffffffu - (uint32_t)top) : 0;
            double* o = out + (size_t)m * 4;
            o[0] = total;
            o[1] = top ? (double)map[idx] : (double)-INFINITY;
            o[2] = (double)(idx % w);
            o[3] = (double)(idx / w);
        }
    }
}

extern "C" int pk_heatmap_summary(const float* heatmaps, double* out, int64_t M, int h, int w, void* stream) {
    PK_REQUIRE(heatmaps && out, "pk_heatmap_summary: null pointer");
    PK_REQUIRE(M > 0 && h > 0 && w > 0 && (int64_t)h * w <= 0x7fffff00, "pk_heatmap_summary: bad shape M=%lld h=%d w=%d", (long long)M, h, w);
    const int gb = capped_grid(M, OCC_MAP_GRID_CAP);
    hipLaunchKernelGGL(k_heatmap_summary, dim3(gb), dim3(OCC_THREADS), 0, (hipStream_t)stream, heatmaps, out, M, h * w, w);
    return pk_launch_status("pk_heatmap_summary");
}

// ================================================================================================ the map
// The reference writes map[i : i + patch, j : j + patch] = base - score position by position, rows outer, columns inner, so the last writer
// of a pixel wins.  Closed form: a = min(y / stride, ny - 1), b = min(x / stride, nx - 1); the pixel is covered iff y < a stride + patch and
// x < b stride + patch and then takes copy a nx + b; otherwise 0 (the bottom and right margins, and the gaps when stride > patch).
// One element of (K, H, W) per thread and pass, every element written exactly once.
__global__ void __launch_bounds__(OCC_THREADS) k_occlusion_paint(const double* __restrict__ base, const double* __restrict__ table,
                                                                 double* __restrict__ maps, int measure, uint32_t K, uint32_t HW, uint32_t W,
                                                                 uint32_t ny, uint32_t nx, uint32_t patch, uint32_t stride, uint64_t total) {
    for (uint64_t i = (uint64_t)blockIdx.x * OCC_THREADS + threadIdx.x; i < total; i += (uint64_t)gridDim.x * OCC_THREADS) {
        const uint32_t j = (uint32_t)i;                           // total < 2^32 - 1 (checked by the entry)
        const uint32_t k = j / HW, r = j - k * HW;
        const uint32_t y = r / W, x = r - y * W;
        uint32_t a = y / stride, b = x / stride;
        a = a < ny - 1 ? a : ny - 1;
        b = b < nx - 1 ? b : nx - 1;
        double v = 0.0;
        if (y - a * stride < patch && x - b * stride < patch) {   // y >= a stride and x >= b stride: no wrap
            const double* __restrict__ t = table + ((size_t)(a * nx + b) * K + k) * 4;
            const double* __restrict__ o = base + (size_t)k * 4;
            if (measure == 0) v = o[0] - t[0];
            else if (measure == 1) v = o[1] - t[1];
            else {
                const double dx = t[2] - o[2], dy = t[3] - o[3];
                v = sqrt(dx * dx + dy * dy);
            }
        }
        maps[i] = v;
    }
}

extern "C" int pk_occlusion_paint(const double* base, const double* table, double* maps, int measure, int K, int H, int W, int patch, int stride,
                                  void* stream) {
    PK_REQUIRE(base && table && maps, "pk_occlusion_paint: null pointer");
    PK_REQUIRE(measure >= 0 && measure <= 2, "pk_occlusion_paint: measure %d (0 sum, 1 max, 2 shift)", measure);
    PK_REQUIRE(K >= 1, "pk_occlusion_paint: bad joint count K=%d", K);
    int ny, nx;
    if (int rc = occ_grid("pk_occlusion_paint", H, W, patch, stride, ny, nx)) return rc;
    PK_REQUIRE((int64_t)H * W < 0xffffffffll / K, "pk_occlusion_paint: %d maps of %d x %d pixels overflow 32-bit indices", K, H, W);
    const size_t total = (size_t)K * H * W;
    unsigned gb;
    if (int rc = chunk_grid(total, 1, CHUNK_GRID_CAP, "pk_occlusion_paint", gb)) return rc;
    hipLaunchKernelGGL(k_occlusion_paint, dim3(gb), dim3(OCC_THREADS), 0, (hipStream_t)stream, base, table, maps, measure, (uint32_t)K,
                       (uint32_t)((int64_t)H * W), (uint32_t)W, (uint32_t)ny, (uint32_t)nx, (uint32_t)patch, (uint32_t)stride, (uint64_t)total);
    return pk_launch_status("pk_occlusion_paint");
}
