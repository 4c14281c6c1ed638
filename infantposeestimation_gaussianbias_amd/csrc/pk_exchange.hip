// The exchange unit: sum of bilinearly up-sampled branches (+ ReLU) and the backward of the up-sampling; single problems and groups.
#include "pk_rowops.h"

// ================================================================================================ exchange-unit sum
// out = relu?( sum_i up_i(x_i) ): every input is NHWC bf16 with the same C; input i has spatial size (H>>s_i, W>>s_i)
// ... in general (Hi, Wi) and is bilinearly up-sampled (align_corners=False) to (H, W) when smaller.
struct FuseIn { const uint16_t* p; int H, W; };
struct FuseArgs { FuseIn in[4]; int n; uint16_t* out; int B, H, W, C, relu; const uint16_t* mask_y; };   // mask_y: term 0 counts only where mask_y > 0
__device__ __forceinline__ void bil_taps(int o, int n_in, int n_out, int& i0, int& i1, float& f) {
    float s = ((float)o + 0.5f) * ((float)n_in / (float)n_out) - 0.5f;
    s = fmaxf(s, 0.f);
    i0 = min((int)s, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    f = s - (float)i0;
}
__device__ __forceinline__ void fuse_sum_body(const FuseArgs& a, const int bid, const int nblocks) {
    const int cchunks = a.C / 8;
    const size_t chunks = (size_t)a.B * a.H * a.W * cchunks;
    const float inv_c = 1.f / (float)cchunks, inv_w = 1.f / (float)a.W, inv_h = 1.f / (float)a.H;
    for (size_t i = (size_t)bid * blockDim.x + threadIdx.x; i < chunks; i += (size_t)nblocks * blockDim.x) {
        // (32-bit index arithmetic: five size_t divisions were ~300 VALU instructions per 16-byte output chunk)
        const uint32_t i32 = (uint32_t)i;
        const bool f24 = chunks < (1u << 24);
        const uint32_t pix0 = f24 ? fdiv24(i32, cchunks, inv_c) : i32 / (uint32_t)cchunks;
        const int cc = (int)(i32 - pix0 * (uint32_t)cchunks);
        const uint32_t pix1 = f24 ? fdiv24(pix0, a.W, inv_w) : pix0 / (uint32_t)a.W;
        const int x = (int)(pix0 - pix1 * (uint32_t)a.W);
        const int b = (int)(f24 ? fdiv24(pix1, a.H, inv_h) : pix1 / (uint32_t)a.H), y = (int)(pix1 - (uint32_t)b * (uint32_t)a.H);
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < a.n; ++k) {
            const FuseIn& in = a.in[k];
            float v[8];
            if (in.H == a.H && in.W == a.W) {
                unpack8(*reinterpret_cast<const uint4*>(in.p + (((size_t)b * a.H + y) * a.W + x) * a.C + cc * 8), v);
                if (k == 0 && a.mask_y) {         // relu backward folded into the sum of input gradients: g = dy * (y > 0)
                    float m[8];
                    unpack8(*reinterpret_cast<const uint4*>(a.mask_y + i * 8), m);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = m[j] > 0.f ? v[j] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += v[j];
            } else {
                int y0, y1, x0, x1;
                float fy, fx;
                bil_taps(y, in.H, a.H, y0, y1, fy);
                bil_taps(x, in.W, a.W, x0, x1, fx);
                const uint16_t* base = in.p + (size_t)b * in.H * in.W * a.C + cc * 8;
                float v01[8], v10[8], v11[8];
                unpack8(*reinterpret_cast<const uint4*>(base + ((size_t)y0 * in.W + x0) * a.C), v);
                unpack8(*reinterpret_cast<const uint4*>(base + ((size_t)y0 * in.W + x1) * a.C), v01);
                unpack8(*reinterpret_cast<const uint4*>(base + ((size_t)y1 * in.W + x0) * a.C), v10);
                unpack8(*reinterpret_cast<const uint4*>(base + ((size_t)y1 * in.W + x1) * a.C), v11);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    acc[j] += (v[j] * (1.f - fx) + v01[j] * fx) * (1.f - fy) + (v10[j] * (1.f - fx) + v11[j] * fx) * fy;
            }
        }
        if (a.relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.f);
        }
        *reinterpret_cast<uint4*>(a.out + i * 8) = pack8(acc);
    }
}
__global__ void __launch_bounds__(256) k_fuse_sum(FuseArgs a) { fuse_sum_body(a, (int)blockIdx.x, (int)gridDim.x); }
struct FuseGroup {
    FuseArgs a[PK_GROUP_MAX];
    int first[PK_GROUP_MAX + 1];
    int n;
};
__global__ void __launch_bounds__(256) k_fuse_sum_g(FuseGroup g) {
    const int L = (int)blockIdx.x;
    PK_GROUP_MEMBER(i, g.first, g.n, L);
    fuse_sum_body(g.a[i], L - g.first[i], g.first[i + 1] - g.first[i]);
}
// One fused-sum problem checked and turned into kernel arguments and a workgroup count (at most `cap`); errors speak as `who`
static int fuse_plan(const PkFuseDesc& c, size_t cap, const char* who, FuseArgs& a, unsigned& blocks) {
    PK_REQUIRE(c.out && c.n_inputs >= 1 && c.n_inputs <= 4, "%s: bad argument", who);
    PK_REQUIRE(c.B > 0 && c.H > 0 && c.W > 0 && c.C > 0 && (c.C & 7) == 0, "%s: bad shape", who);
    for (int i = 0; i < c.n_inputs; ++i) {
        PK_REQUIRE(c.inputs[i] && c.in_h[i] > 0 && c.in_w[i] > 0 && c.in_h[i] <= c.H && c.in_w[i] <= c.W, "%s: input %d shape", who, i);
        a.in[i] = FuseIn{(const uint16_t*)c.inputs[i], c.in_h[i], c.in_w[i]};
    }
    PK_REQUIRE(!c.mask_y || (c.in_h[0] == c.H && c.in_w[0] == c.W), "%s: the masked term must have the output's size", who);
    a.n = c.n_inputs; a.out = (uint16_t*)c.out; a.B = c.B; a.H = c.H; a.W = c.W; a.C = c.C; a.relu = c.relu; a.mask_y = (const uint16_t*)c.mask_y;
    return chunk_grid((size_t)c.B * c.H * c.W * (c.C / 8), 1, cap, who, blocks);
}
// up to PK_GROUP_MAX sums (the outputs of one exchange unit, or the input-gradient sums of its backward) in ONE launch
extern "C" int pk_fuse_sum_group(const PkFuseDesc* d, int n, void* stream) {
    PK_REQUIRE(d && n > 0 && n <= PK_GROUP_MAX, "pk_fuse_sum_group: 1..%d members, got %d", PK_GROUP_MAX, n);
    FuseGroup g{};
    int total = 0;
    for (int i = 0; i < n; ++i) {
        unsigned gb;
        if (int rc = fuse_plan(d[i], CHUNK_GRID_CAP_GROUPED, "pk_fuse_sum_group", g.a[i], gb)) return rc;
        g.first[i] = total;
        total += (int)gb;
    }
    g.first[n] = total;
    g.n = n;
    hipLaunchKernelGGL(k_fuse_sum_g, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, g);
    return pk_launch_status("pk_fuse_sum_group");
}
extern "C" int pk_fuse_sum(const void* const* inputs, const int* in_h, const int* in_w, int n_inputs, void* out, int B, int H, int W,
                           int C, int relu, void* stream) {
    PK_REQUIRE(inputs && in_h && in_w && out && n_inputs >= 1 && n_inputs <= 4, "pk_fuse_sum: bad argument");
    PkFuseDesc c{};
    for (int i = 0; i < n_inputs; ++i) {
        c.inputs[i] = inputs[i];
        c.in_h[i] = in_h[i];
        c.in_w[i] = in_w[i];
    }
    c.n_inputs = n_inputs; c.out = out; c.B = B; c.H = H; c.W = W; c.C = C; c.relu = relu;
    FuseArgs a{};
    unsigned gb;
    if (int rc = fuse_plan(c, CHUNK_GRID_CAP, "pk_fuse_sum", a, gb)) return rc;
    hipLaunchKernelGGL(k_fuse_sum, dim3(gb), dim3(256), 0, (hipStream_t)stream, a);
    return pk_launch_status("pk_fuse_sum");
}

// Backward of the bilinear up-sampling (gather form, deterministic): dsrc[b][ys][xs][c] = sum over the output pixels
// whose taps touch (ys,xs) of weight * dy.  `dy` is the (already relu-masked) gradient at the fused resolution.
template <int SPLIT>   // lanes that share one output chunk (each takes every SPLIT-th row of the gather window)
__device__ __forceinline__ void upsample_bwd_body(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ mask_y, uint16_t* __restrict__ dsrc,
                                                  int B, int H, int W, int Hs, int Ws, int C, const int bid, const int nblocks) {
    const int cchunks = C / 8;
    const size_t chunks = (size_t)B * Hs * Ws * cchunks;
    const int ry = (H + Hs - 1) / Hs, rx = (W + Ws - 1) / Ws;
    const int sub = threadIdx.x % SPLIT;
    const size_t groups_per_grid = (size_t)nblocks * blockDim.x / SPLIT;
    const size_t n_iter = (chunks + groups_per_grid - 1) / groups_per_grid;          // uniform trip count: all lanes reach the shuffles
    size_t i = ((size_t)bid * blockDim.x + threadIdx.x) / SPLIT;
    for (size_t it = 0; it < n_iter; ++it, i += groups_per_grid) {
        const bool on = i < chunks;
        const size_t ii = on ? i : 0;
        const uint32_t i32 = (uint32_t)ii;
        const bool f24 = chunks < (1u << 24);
        const uint32_t pix0 = f24 ? fdiv24(i32, cchunks, 1.f / (float)cchunks) : i32 / (uint32_t)cchunks;
        const int cc = (int)(i32 - pix0 * (uint32_t)cchunks);
        const uint32_t pix1 = f24 ? fdiv24(pix0, Ws, 1.f / (float)Ws) : pix0 / (uint32_t)Ws;
        const int xs = (int)(pix0 - pix1 * (uint32_t)Ws);
        const int b = (int)(f24 ? fdiv24(pix1, Hs, 1.f / (float)Hs) : pix1 / (uint32_t)Hs), ys = (int)(pix1 - (uint32_t)b * (uint32_t)Hs);
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // support of source pixel ys: outputs whose source coordinate (oy + .5) * Hs/H - .5 lies in (ys-1, ys+1), i.e.
        // oy in ((ys-.5)*H/Hs - .5, (ys+1.5)*H/Hs - .5); H/Hs <= ry, one extra row each side covers non-integer ratios.
        // (The border clamps only move outputs that are already inside this range.)
        // For an exact even ratio r the support is EXACTLY the 2r outputs [ys r - r/2, ys r + 3r/2): the generic window above scans
        // 3r + 2 candidates per axis and computes the taps of each (r = 2: 64 candidates for 16 contributors -- the kernel was bound by
        // that arithmetic, ~19 us for a 6 MB gradient).
        const bool ey = (H == Hs * ry) && !(ry & 1), ex = (W == Ws * rx) && !(rx & 1);
        const int oy_lo = ey ? max(0, ys * ry - ry / 2) : max(0, (ys - 1) * ry - 1), oy_hi = ey ? min(H, ys * ry + 3 * ry / 2) : min(H, (ys + 2) * ry + 1);
        const int ox_lo = ex ? max(0, xs * rx - rx / 2) : max(0, (xs - 1) * rx - 1), ox_hi = ex ? min(W, xs * rx + 3 * rx / 2) : min(W, (xs + 2) * rx + 1);
        if (on)
            for (int oy = oy_lo + sub; oy < oy_hi; oy += SPLIT) {
                int y0, y1;
                float fy;
                bil_taps(oy, Hs, H, y0, y1, fy);
                const float wy = (y0 == ys ? 1.f - fy : 0.f) + (y1 == ys ? fy : 0.f);
                if (wy == 0.f) continue;
                for (int ox = ox_lo; ox < ox_hi; ++ox) {
                    int x0, x1;
                    float fx;
                    bil_taps(ox, Ws, W, x0, x1, fx);
                    const float wx = (x0 == xs ? 1.f - fx : 0.f) + (x1 == xs ? fx : 0.f);
                    if (wx == 0.f) continue;
                    float v[8];
                    unpack8(*reinterpret_cast<const uint4*>(dy + (((size_t)b * H + oy) * W + ox) * C + cc * 8), v);
                    if (mask_y) {                 // relu backward of the fused sum folded in: the gradient counts only where y > 0
                        float m[8];
                        unpack8(*reinterpret_cast<const uint4*>(mask_y + (((size_t)b * H + oy) * W + ox) * C + cc * 8), m);
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = m[j] > 0.f ? v[j] : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += wy * wx * v[j];
                }
            }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = lanes_sum<SPLIT>(acc[j]);       // fixed butterfly over the SPLIT row-lanes: deterministic
        if (on && sub == 0) *reinterpret_cast<uint4*>(dsrc + i * 8) = pack8(acc);
    }
}
template <int SPLIT>
__global__ void __launch_bounds__(256) k_upsample_bwd(const uint16_t* __restrict__ dy, uint16_t* __restrict__ dsrc, int B, int H, int W,
                                                      int Hs, int Ws, int C) {
    upsample_bwd_body<SPLIT>(dy, nullptr, dsrc, B, H, W, Hs, Ws, C, (int)blockIdx.x, (int)gridDim.x);
}
// One up-sampling-backward problem checked; `split`: lanes per output chunk, `blocks`: its workgroups (at most `cap`); errors speak as `who`
static int upsample_plan(const PkUpBwdDesc& c, size_t cap, const char* who, int& split, unsigned& blocks) {
    PK_REQUIRE(c.dy && c.dsrc && c.B > 0 && c.H >= c.Hs && c.W >= c.Ws && c.Hs > 0 && c.Ws > 0 && c.C > 0 && (c.C & 7) == 0, "%s: bad argument", who);
    const size_t chunks = (size_t)c.B * c.Hs * c.Ws * (c.C / 8);
    const int ry = (c.H + c.Hs - 1) / c.Hs;
    // few output chunks with a tall gather window (scale 4 / 8): spread the window rows over 4 / 16 lanes per chunk
    split = (ry >= 8 && chunks < (1u << 20)) ? 16 : ((ry >= 4 && chunks < (1u << 20)) ? 4 : 1);
    return chunk_grid(chunks, split, cap, who, blocks);
}
struct UpBwdGroup {
    PkUpBwdDesc d[PK_GROUP_MAX];
    int first[PK_GROUP_MAX + 1], split[PK_GROUP_MAX];
    int n;
};
__global__ void __launch_bounds__(256) k_upsample_bwd_g(UpBwdGroup g) {
    const int L = (int)blockIdx.x;
    PK_GROUP_MEMBER(i, g.first, g.n, L);
    const PkUpBwdDesc& d = g.d[i];
    const int bid = L - g.first[i], nb = g.first[i + 1] - g.first[i], sp = g.split[i];
    const uint16_t* dy = (const uint16_t*)d.dy;
    const uint16_t* my = (const uint16_t*)d.mask_y;
    uint16_t* ds = (uint16_t*)d.dsrc;
    if (sp == 16) upsample_bwd_body<16>(dy, my, ds, d.B, d.H, d.W, d.Hs, d.Ws, d.C, bid, nb);
    else if (sp == 4) upsample_bwd_body<4>(dy, my, ds, d.B, d.H, d.W, d.Hs, d.Ws, d.C, bid, nb);
    else upsample_bwd_body<1>(dy, my, ds, d.B, d.H, d.W, d.Hs, d.Ws, d.C, bid, nb);
}
// the up-sampling backward of every up-route of one exchange unit in ONE launch; mask_y (optional) folds the fused sum's ReLU backward in
extern "C" int pk_upsample_bwd_group(const PkUpBwdDesc* d, int n, void* stream) {
    PK_REQUIRE(d && n > 0 && n <= PK_GROUP_MAX, "pk_upsample_bwd_group: 1..%d members, got %d", PK_GROUP_MAX, n);
    UpBwdGroup g{};
    int total = 0;
    for (int i = 0; i < n; ++i) {
        unsigned gb;
        if (int rc = upsample_plan(d[i], CHUNK_GRID_CAP_GROUPED, "pk_upsample_bwd_group", g.split[i], gb)) return rc;
        g.d[i] = d[i];
        g.first[i] = total;
        total += (int)gb;
    }
    g.first[n] = total;
    g.n = n;
    hipLaunchKernelGGL(k_upsample_bwd_g, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, g);
    return pk_launch_status("pk_upsample_bwd_group");
}
extern "C" int pk_sizeof_group_desc(int which) {
    switch (which) {
        case 0: return (int)sizeof(PkConvDesc);
        case 1: return (int)sizeof(PkBnFwdDesc);
        case 2: return (int)sizeof(PkBnBwdDesc);
        case 3: return (int)sizeof(PkFuseDesc);
        case 4: return (int)sizeof(PkUpBwdDesc);
        case 5: return (int)sizeof(PkWgradDesc);
        default: return -1;
    }
}
extern "C" int pk_upsample_bilinear_bwd(const void* dy, void* dsrc, int B, int H, int W, int Hs, int Ws, int C, void* stream) {
    PkUpBwdDesc c{};
    c.dy = dy; c.dsrc = dsrc; c.B = B; c.H = H; c.W = W; c.Hs = Hs; c.Ws = Ws; c.C = C;
    int split;
    unsigned gb;
    if (int rc = upsample_plan(c, CHUNK_GRID_CAP, "pk_upsample_bilinear_bwd", split, gb)) return rc;
#define UP_LAUNCH(SPLIT) hipLaunchKernelGGL(k_upsample_bwd<SPLIT>, dim3(gb), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)dy, (uint16_t*)dsrc, B, H, W, Hs, Ws, C)
    if (split == 16) UP_LAUNCH(16);
    else if (split == 4) UP_LAUNCH(4);
    else UP_LAUNCH(1);
#undef UP_LAUNCH
    return pk_launch_status("pk_upsample_bilinear_bwd");
}
