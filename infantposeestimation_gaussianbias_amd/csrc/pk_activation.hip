// Activation statistics of an NHWC bf16 feature map seen as M rows x C channels (this project's own specification: DESIGN.md "Activation
// statistics"; the numbers behind the reference's ActivationAnalyzer, analysis/advanced_analysis.py:34-125, which copies every tapped
// tensor to the host and sorts it there).  Two entries:
//   pk_activation_stats      k_act_stats_partial: every workgroup strides over slabs of rows with 16-byte loads, eight channels per thread in
//                            registers, the 4096-bin table as int32 LDS atomicAdd counts; k_act_stats_finalize: 16 threads per channel and
//                            per bin over the workgroups' partials, each in ascending workgroup order, then those 16 from left to right.
//   pk_activation_quantiles  k_act_rank_bins (which bin holds each rank), k_act_sub_bins (one more pass over x: the 16 sub-bins of the selected
//                            bins), k_act_pick (the values).  A bin and a sub-bin are the 16 bits of a bf16: the select is exact.
// No global atomics, no float atomics, no last-arriver.  Counts are integers (order-free); min / max run over finite values with -0 read as
// +0 (order-free); the two fp64 sums are taken in the order written at act_fold and k_act_stats_finalize, which (M, C) alone fix.
#include "pk_common.h"

#include <math.h>

#define ACT_THREADS 256
#define ACT_WAVES (ACT_THREADS / PK_WAVE)
#define ACT_UNROLL 4                       // 16-byte loads in flight per thread
#define ACT_MAX_BLOCKS 512                 // two workgroups per compute unit; bounds the partials (36 C + 16 400 bytes per workgroup)
#define ACT_BINS PK_ACT_HIST_BINS
#define ACT_ZERO_BIN 2048                  // key(+0) = 0x8000, >> 4
#define ACT_HIST_STRIDE (ACT_BINS + 4)     // int32 per workgroup: the bins, then the workgroup's count of +-0 (which never enter LDS), padding
#define ACT_TARGETS (2 * PK_ACT_MAX_QUANTILES)
#define ACT_SUB_STRIDE (ACT_TARGETS * 16 + 4)

struct __attribute__((aligned(16))) ActRecord {
    double sum, sumsq;
    float mn, mx;
    int64_t n, n_zero, n_negative, n_nonfinite, reserved;
};
static_assert(sizeof(ActRecord) == PK_ACT_RECORD_BYTES, "record layout");
struct __attribute__((aligned(16))) ActSel { int32_t bin, slot; int64_t rank; };      // bin < 0: no finite element
struct ActQ { double q[PK_ACT_MAX_QUANTILES]; };

// The split of rows over workgroups, a function of (M, C) alone.  CH = C / 8 threads cover one row, G = 256 / CH rows are read per pass
// (threads >= G CH idle), a slab is ACT_UNROLL passes, workgroup b of B = min(512, ceil(M / slab)) takes slabs b, b + B, ...
// Thread t = r CH + c owns channels 8 c .. 8 c + 7 of rows s slab + u G + r, in ascending (s, u).
static inline int act_rows_per_pass(int C) { return ACT_THREADS / (C / 8); }
static inline int64_t act_slab(int C) { return (int64_t)act_rows_per_pass(C) * ACT_UNROLL; }
static inline int act_blocks(int64_t M, int C) { return capped_grid((M + act_slab(C) - 1) / act_slab(C), ACT_MAX_BLOCKS); }

// partials, structure of arrays over [workgroup][channel]: sum, sumsq f64; min, max f32; zero, negative, nonfinite u32; then the tables
struct ActWs {
    double *sum, *sumsq;
    float *mn, *mx;
    uint32_t *nz, *ng, *nf;
    int32_t* hist;
};
__host__ __device__ static inline ActWs act_ws(void* ws, int blocks, int C) {
    char* p = reinterpret_cast<char*>(ws);
    const size_t bc = (size_t)blocks * C;
    ActWs w;
    w.sum = reinterpret_cast<double*>(p);
    w.sumsq = reinterpret_cast<double*>(p + 8 * bc);
    w.mn = reinterpret_cast<float*>(p + 16 * bc);
    w.mx = reinterpret_cast<float*>(p + 20 * bc);
    w.nz = reinterpret_cast<uint32_t*>(p + 24 * bc);
    w.ng = reinterpret_cast<uint32_t*>(p + 28 * bc);
    w.nf = reinterpret_cast<uint32_t*>(p + 32 * bc);
    w.hist = reinterpret_cast<int32_t*>(p + 36 * bc);
    return w;
}
static inline int64_t act_ws_bytes(int blocks, int C) { return (int64_t)blocks * (36 * (int64_t)C + 4 * ACT_HIST_STRIDE); }

// sortable key of a finite bf16 that is not -0: ascending key == ascending value
__device__ __forceinline__ uint32_t act_key(uint32_t h) { return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u); }
__device__ __forceinline__ float act_value_of_key(uint32_t key) {
    const uint32_t h = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
    return __uint_as_float(h << 16);
}

// Workgroup fold of one field: thread t = r CH + c parks its eight values at s[r C + 8 c + e]; channel j takes s[j] op s[C + j] op ... op
// s[(G - 1) C + j] from left to right and goes to out[j].  Barriers on both sides.
template <class V, class Op>
__device__ __forceinline__ void act_fold(V* s, const V (&a)[8], bool active, int G, int C, V* __restrict__ out, Op op) {
    if (active) {
#pragma unroll
        for (int e = 0; e < 8; ++e) s[threadIdx.x * 8 + e] = a[e];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < C; j += ACT_THREADS) {
        V acc = s[j];
        for (int r = 1; r < G; ++r) acc = op(acc, s[r * C + j]);
        out[j] = acc;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(ACT_THREADS) k_act_stats_partial(const u32x4* __restrict__ x, int64_t M, int CH, int G, int c_used, void* ws) {
    __shared__ int s_hist[ACT_BINS];
    __shared__ double s_red[ACT_THREADS * 8];
    __shared__ int red_i[ACT_WAVES];
    const int t = threadIdx.x, C = CH * 8, blocks = gridDim.x, b = blockIdx.x;
    for (int i = t; i < ACT_BINS; i += ACT_THREADS) s_hist[i] = 0;
    __syncthreads();
    const bool active = t < G * CH;
    const int r = t / CH, c = t - r * CH;
    const int lim = c_used - 8 * c;                                // elements e < lim of this thread's chunk are real channels
    double sum[8], sq[8];
    float mn[8], mx[8];
    uint32_t nz[8], ng[8], nf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] = sq[e] = 0.0, mn[e] = INFINITY, mx[e] = -INFINITY, nz[e] = ng[e] = nf[e] = 0u;
    const int64_t slab = (int64_t)G * ACT_UNROLL;
    for (int64_t s = b; s * slab < M; s += blocks) {
        u32x4 v[ACT_UNROLL];
        bool ok[ACT_UNROLL];
#pragma unroll
        for (int u = 0; u < ACT_UNROLL; ++u) {
            const int64_t row = s * slab + (int64_t)u * G + r;
            ok[u] = active && row < M;
            if (ok[u]) v[u] = x[row * CH + c];
        }
#pragma unroll
        for (int u = 0; u < ACT_UNROLL; ++u) {
            if (!ok[u]) continue;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t w = v[u][e >> 1], h = (e & 1) ? (w >> 16) : (w & 0xffffu);
                if (e >= lim) continue;                            // padding channel
                if ((h & 0x7f80u) == 0x7f80u) {                    // exponent bits all ones: inf / NaN (pk_tensor_stats' rule)
                    nf[e] += 1;
                } else if ((h & 0x7fffu) == 0u) {                  // +-0: counted here, min / max see +0, never through the LDS table
                    nz[e] += 1;
                    mn[e] = fminf(mn[e], 0.f);
                    mx[e] = fmaxf(mx[e], 0.f);
                } else {
                    const float f = __uint_as_float(h << 16);
                    const double d = (double)f;
                    sum[e] += d;
                    sq[e] += d * d;
                    mn[e] = fminf(mn[e], f);
                    mx[e] = fmaxf(mx[e], f);
                    ng[e] += h >> 15;
                    atomicAdd(&s_hist[act_key(h) >> 4], 1);        // integer counts in LDS: order-free
                }
            }
        }
    }
    const ActWs w = act_ws(ws, blocks, C);
    const size_t o = (size_t)b * C;
    act_fold(s_red, sum, active, G, C, w.sum + o, SumOp());
    act_fold(s_red, sq, active, G, C, w.sumsq + o, SumOp());
    act_fold(reinterpret_cast<float*>(s_red), mn, active, G, C, w.mn + o, MinOp());
    act_fold(reinterpret_cast<float*>(s_red), mx, active, G, C, w.mx + o, MaxOp());
    act_fold(reinterpret_cast<uint32_t*>(s_red), nz, active, G, C, w.nz + o, SumOp());
    act_fold(reinterpret_cast<uint32_t*>(s_red), ng, active, G, C, w.ng + o, SumOp());
    act_fold(reinterpret_cast<uint32_t*>(s_red), nf, active, G, C, w.nf + o, SumOp());
    int zeros = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) zeros += (int)nz[e];
    zeros = block_reduce<ACT_WAVES>(zeros, red_i, SumOp());        // its first barrier also orders the LDS atomics before the copy below
    int32_t* hp = w.hist + (size_t)b * ACT_HIST_STRIDE;
    for (int i = t; i < ACT_BINS; i += ACT_THREADS) hp[i] = s_hist[i];
    if (t == 0) hp[ACT_BINS] = zeros;
}

// The partials of B workgroups are folded by 16 groups of 16 threads: group g adds workgroups g, g + 16, g + 32, ... in ascending order to
// 0.0 (independent loads, a few round trips instead of B), then the groups 0, 1, ..., 15 are added from left to right through LDS.
// Workgroups 0 .. 255 of this kernel take 16 bins each (the zero bin also takes the workgroups' zero counts), the ones behind them 16
// channels each.  accumulate: old + new per field, min / max combined.
#define ACT_FOLD 16
__global__ void __launch_bounds__(ACT_THREADS) k_act_stats_finalize(void* ws, int blocks, int C, int c_used, int64_t M, int accumulate,
                                                                    ActRecord* __restrict__ records, int64_t* __restrict__ hist) {
    __shared__ double s_sum[ACT_THREADS], s_sq[ACT_THREADS];
    __shared__ float s_mn[ACT_THREADS], s_mx[ACT_THREADS];
    __shared__ long long s_cnt[3][ACT_THREADS];
    const int t = threadIdx.x, l = t & (ACT_FOLD - 1), g = t / ACT_FOLD;
    const ActWs w = act_ws(ws, blocks, C);
    if (blockIdx.x < ACT_BINS / ACT_FOLD) {                       // uniform over the workgroup
        const int bin = blockIdx.x * ACT_FOLD + l;
        long long n = 0;
#pragma unroll 8
        for (int b = g; b < blocks; b += ACT_FOLD) n += w.hist[(size_t)b * ACT_HIST_STRIDE + bin];
        if (bin == ACT_ZERO_BIN) {
#pragma unroll 8
            for (int b = g; b < blocks; b += ACT_FOLD) n += w.hist[(size_t)b * ACT_HIST_STRIDE + ACT_BINS];
        }
        s_cnt[0][t] = n;
        __syncthreads();
        if (g == 0) {
            long long tot = 0;
            for (int k = 0; k < ACT_FOLD; ++k) tot += s_cnt[0][k * ACT_FOLD + l];
            hist[bin] = (accumulate ? hist[bin] : 0) + tot;
        }
        return;
    }
    const int j = (blockIdx.x - ACT_BINS / ACT_FOLD) * ACT_FOLD + l;
    const bool live = j < c_used;
    double sum = 0.0, sq = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    long long nz = 0, ng = 0, nf = 0;
    if (live) {
#pragma unroll 4
        for (int b = g; b < blocks; b += ACT_FOLD) {
            const size_t i = (size_t)b * C + j;
            sum += w.sum[i];
            sq += w.sumsq[i];
            mn = fminf(mn, w.mn[i]);
            mx = fmaxf(mx, w.mx[i]);
            nz += w.nz[i];
            ng += w.ng[i];
            nf += w.nf[i];
        }
    }
    s_sum[t] = sum, s_sq[t] = sq, s_mn[t] = mn, s_mx[t] = mx, s_cnt[0][t] = nz, s_cnt[1][t] = ng, s_cnt[2][t] = nf;
    __syncthreads();
    if (g != 0 || !live) return;
    ActRecord r = {s_sum[l], s_sq[l], s_mn[l], s_mx[l], M, s_cnt[0][l], s_cnt[1][l], s_cnt[2][l], 0};
    for (int k = 1; k < ACT_FOLD; ++k) {
        const int i = k * ACT_FOLD + l;
        r.sum += s_sum[i];
        r.sumsq += s_sq[i];
        r.mn = fminf(r.mn, s_mn[i]);
        r.mx = fmaxf(r.mx, s_mx[i]);
        r.n_zero += s_cnt[0][i];
        r.n_negative += s_cnt[1][i];
        r.n_nonfinite += s_cnt[2][i];
    }
    if (accumulate) {
        const ActRecord o = records[j];
        r.sum = o.sum + r.sum;
        r.sumsq = o.sumsq + r.sumsq;
        r.mn = fminf(o.mn, r.mn);
        r.mx = fmaxf(o.mx, r.mx);
        r.n += o.n;
        r.n_zero += o.n_zero;
        r.n_negative += o.n_negative;
        r.n_nonfinite += o.n_nonfinite;
    }
    records[j] = r;
}

// ================================================================================================ exact order statistics
// Target 2 i: rank lo of quantile i, target 2 i + 1: rank hi.  One workgroup; thread t owns bins 16 t .. 16 t + 15 of the table.
__global__ void __launch_bounds__(ACT_THREADS) k_act_rank_bins(const int64_t* __restrict__ hist, ActQ qs, int Q, ActSel* __restrict__ sel) {
    __shared__ long long s_sum[ACT_THREADS];
    __shared__ int s_bin[ACT_TARGETS];
    const int t = threadIdx.x;
    long long h[16], mine = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) h[i] = hist[16 * t + i], mine += h[i];
    s_sum[t] = mine;
    if (t < ACT_TARGETS) s_bin[t] = -1;
    __syncthreads();
    long long excl = 0, n = 0;
    for (int i = 0; i < ACT_THREADS; ++i) {
        if (i == t) excl = n;
        n += s_sum[i];
    }
    if (n > 0) {
        for (int k = 0; k < 2 * Q; ++k) {
            const double pos = qs.q[k >> 1] * (double)(n - 1);
            const long long lo = pos >= 0.0 ? (pos < (double)(n - 1) ? (long long)floor(pos) : n - 1) : 0;
            const long long rank = (k & 1) ? (lo + 1 < n ? lo + 1 : n - 1) : lo;
            if (rank < excl || rank >= excl + mine) continue;
            long long below = excl;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (rank >= below && rank < below + h[i]) {
                    sel[k].bin = 16 * t + i;
                    sel[k].rank = rank - below;
                    s_bin[k] = 16 * t + i;
                }
                below += h[i];
            }
        }
    }
    __syncthreads();
    if (t < 2 * Q) {                                               // targets in one bin share the slot of the first of them
        int slot = t;
        for (int k = t - 1; k >= 0; --k)
            if (s_bin[k] == s_bin[t]) slot = k;
        sel[t].slot = slot;
        if (s_bin[t] < 0) sel[t].bin = -1, sel[t].rank = 0;
    }
}

// The pass of k_act_stats_partial again, counting the low four key bits of the elements that fall into a selected bin.
__global__ void __launch_bounds__(ACT_THREADS) k_act_sub_bins(const u32x4* __restrict__ x, int64_t M, int CH, int G, int c_used, int n_targets,
                                                              const ActSel* __restrict__ sel, int32_t* __restrict__ part) {
    __shared__ uint8_t s_lut[ACT_BINS];
    __shared__ int s_sub[ACT_TARGETS * 16];
    __shared__ int red_i[ACT_WAVES];
    const int t = threadIdx.x, blocks = gridDim.x, b = blockIdx.x;
    for (int i = t; i < ACT_BINS; i += ACT_THREADS) s_lut[i] = 0xff;
    for (int i = t; i < ACT_TARGETS * 16; i += ACT_THREADS) s_sub[i] = 0;
    __syncthreads();
    if (t < n_targets) {
        const ActSel s = sel[t];
        if (s.bin >= 0 && s.slot == t) s_lut[s.bin] = (uint8_t)t;
    }
    __syncthreads();
    const bool active = t < G * CH;
    const int r = t / CH, c = t - r * CH;
    const int lim = c_used - 8 * c;
    int zeros = 0;
    const int64_t slab = (int64_t)G * ACT_UNROLL;
    for (int64_t s = b; s * slab < M; s += blocks) {
        u32x4 v[ACT_UNROLL];
        bool ok[ACT_UNROLL];
#pragma unroll
        for (int u = 0; u < ACT_UNROLL; ++u) {
            const int64_t row = s * slab + (int64_t)u * G + r;
            ok[u] = active && row < M;
            if (ok[u]) v[u] = x[row * CH + c];
        }
#pragma unroll
        for (int u = 0; u < ACT_UNROLL; ++u) {
            if (!ok[u]) continue;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t w = v[u][e >> 1], h = (e & 1) ? (w >> 16) : (w & 0xffffu);
                if (e >= lim || (h & 0x7f80u) == 0x7f80u) continue;
                if ((h & 0x7fffu) == 0u) {
                    zeros += 1;
                    continue;
                }
                const uint32_t key = act_key(h), slot = s_lut[key >> 4];
                if (slot != 0xffu) atomicAdd(&s_sub[slot * 16 + (key & 15u)], 1);
            }
        }
    }
    zeros = block_reduce<ACT_WAVES>(zeros, red_i, SumOp());
    int32_t* p = part + (size_t)b * ACT_SUB_STRIDE;
    for (int i = t; i < ACT_TARGETS * 16; i += ACT_THREADS) p[i] = s_sub[i];
    if (t == 0) p[ACT_TARGETS * 16] = zeros;
}

// One workgroup per target: 16 groups of 16 threads fold the workgroups' counts of the 16 sub-bins of the target's slot (group g takes
// workgroups g, g + 16, ...), then thread 0 walks the sub-bins.  Integers: order-free.
__global__ void __launch_bounds__(ACT_THREADS) k_act_pick(const ActSel* __restrict__ sel, const int32_t* __restrict__ part, int blocks,
                                                          float* __restrict__ order) {
    __shared__ long long s_n[ACT_THREADS];
    const int t = threadIdx.x, sub = t & 15, g = t >> 4, k = blockIdx.x;
    const ActSel s = sel[k];
    if (s.bin < 0) {                                              // uniform over the workgroup: no finite element
        if (t == 0) order[k] = __builtin_nanf("");
        return;
    }
    long long n = 0;
#pragma unroll 8
    for (int b = g; b < blocks; b += 16) n += part[(size_t)b * ACT_SUB_STRIDE + s.slot * 16 + sub];
    if (sub == 0 && s.bin == ACT_ZERO_BIN) {                      // +0 is sub-bin 0 of its bin
#pragma unroll 8
        for (int b = g; b < blocks; b += 16) n += part[(size_t)b * ACT_SUB_STRIDE + ACT_TARGETS * 16];
    }
    s_n[t] = n;
    __syncthreads();
    if (t != 0) return;
    float v = __builtin_nanf("");
    long long below = 0;
    for (int i = 0; i < 16; ++i) {
        long long c = 0;
        for (int q = 0; q < 16; ++q) c += s_n[q * 16 + i];
        if (s.rank >= below && s.rank < below + c) v = act_value_of_key(((uint32_t)s.bin << 4) | (uint32_t)i);
        below += c;
    }
    order[k] = v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static int act_check_shape(const char* who, int64_t M, int C, int c_used) {
    PK_REQUIRE(C % 8 == 0, "%s: C=%d must be a multiple of 8 (16-byte bf16 chunks)", who, C);
    PK_REQUIRE(C >= 8 && C <= PK_ACT_MAX_CHANNELS, "%s: C=%d outside [8, %d]", who, C, PK_ACT_MAX_CHANNELS);
    PK_REQUIRE(c_used >= 1 && c_used <= C, "%s: c_used=%d outside [1, C=%d]", who, c_used, C);
    PK_REQUIRE(M >= 1 && M <= PK_ACT_MAX_ELEMS / C, "%s: M=%lld rows of C=%d: M C outside [1, 2^38]", who, (long long)M, C);
    return PK_OK;
}

extern "C" int pk_activation_stats_slab(int C) {
    if (int rc = act_check_shape("pk_activation_stats_slab", 1, C, 1)) return rc;
    return (int)act_slab(C);
}

extern "C" int pk_activation_stats_blocks(int64_t M, int C) {
    if (act_check_shape("pk_activation_stats_blocks", M, C, 1)) return 0;      // a count: no workgroups for a refused shape, the text is set
    return act_blocks(M, C);
}

extern "C" int pk_activation_stats_ws_bytes(int64_t M, int C) {
    if (int rc = act_check_shape("pk_activation_stats_ws_bytes", M, C, 1)) return rc;
    return (int)act_ws_bytes(act_blocks(M, C), C);
}

extern "C" int pk_activation_quantiles_ws_bytes(int64_t M, int C) {
    if (int rc = act_check_shape("pk_activation_quantiles_ws_bytes", M, C, 1)) return rc;
    return (int)(sizeof(ActSel) * ACT_TARGETS + 4 * (int64_t)ACT_SUB_STRIDE * act_blocks(M, C));
}

extern "C" int pk_activation_stats(const void* x, int64_t M, int C, int c_used, void* ws, int64_t ws_bytes, void* records, int64_t* hist,
                                   int accumulate, void* stream) {
    PK_REQUIRE(x && ws && records && hist, "pk_activation_stats: null pointer");
    if (int rc = act_check_shape("pk_activation_stats", M, C, c_used)) return rc;
    PK_REQUIRE((((uintptr_t)x | (uintptr_t)ws | (uintptr_t)records) & 15) == 0 && ((uintptr_t)hist & 7) == 0,
               "pk_activation_stats: misaligned buffer (x, ws, records: 16 bytes; hist: 8)");
    const int blocks = act_blocks(M, C);
    PK_REQUIRE(ws_bytes >= act_ws_bytes(blocks, C), "pk_activation_stats: ws_bytes=%lld, but M=%lld C=%d need %lld (pk_activation_stats_ws_bytes)",
               (long long)ws_bytes, (long long)M, C, (long long)act_ws_bytes(blocks, C));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_act_stats_partial, dim3(blocks), dim3(ACT_THREADS), 0, s, reinterpret_cast<const u32x4*>(x), M, C / 8,
                       act_rows_per_pass(C), c_used, ws);
    if (int rc = pk_launch_status("pk_activation_stats")) return rc;
    hipLaunchKernelGGL(k_act_stats_finalize, dim3(ACT_BINS / ACT_FOLD + (c_used + ACT_FOLD - 1) / ACT_FOLD), dim3(ACT_THREADS), 0, s, ws, blocks, C,
                       c_used, M, accumulate, reinterpret_cast<ActRecord*>(records), hist);
    return pk_launch_status("pk_activation_stats");
}

extern "C" int pk_activation_quantiles(const void* x, int64_t M, int C, int c_used, const int64_t* hist, const double* q_host, int Q, void* ws,
                                       int64_t ws_bytes, float* order, void* stream) {
    PK_REQUIRE(x && hist && q_host && ws && order, "pk_activation_quantiles: null pointer");
    if (int rc = act_check_shape("pk_activation_quantiles", M, C, c_used)) return rc;
    PK_REQUIRE(Q >= 1 && Q <= PK_ACT_MAX_QUANTILES, "pk_activation_quantiles: %d quantiles (1 to %d)", Q, PK_ACT_MAX_QUANTILES);
    ActQ qs = {};
    for (int i = 0; i < Q; ++i) {
        PK_REQUIRE(q_host[i] >= 0.0 && q_host[i] <= 1.0, "pk_activation_quantiles: q[%d]=%g outside [0, 1]", i, q_host[i]);      // false for NaN too
        qs.q[i] = q_host[i];
    }
    PK_REQUIRE((((uintptr_t)x | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)hist & 7) == 0 && ((uintptr_t)order & 3) == 0,
               "pk_activation_quantiles: misaligned buffer (x, ws: 16 bytes; hist: 8; order: 4)");
    const int blocks = act_blocks(M, C);
    const int64_t need = (int64_t)sizeof(ActSel) * ACT_TARGETS + 4 * (int64_t)ACT_SUB_STRIDE * blocks;
    PK_REQUIRE(ws_bytes >= need, "pk_activation_quantiles: ws_bytes=%lld, but M=%lld C=%d need %lld (pk_activation_quantiles_ws_bytes)",
               (long long)ws_bytes, (long long)M, C, (long long)need);
    ActSel* sel = reinterpret_cast<ActSel*>(ws);
    int32_t* part = reinterpret_cast<int32_t*>(sel + ACT_TARGETS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_act_rank_bins, dim3(1), dim3(ACT_THREADS), 0, s, hist, qs, Q, sel);
    if (int rc = pk_launch_status("pk_activation_quantiles")) return rc;
    hipLaunchKernelGGL(k_act_sub_bins, dim3(blocks), dim3(ACT_THREADS), 0, s, reinterpret_cast<const u32x4*>(x), M, C / 8, act_rows_per_pass(C),
                       c_used, 2 * Q, sel, part);
    if (int rc = pk_launch_status("pk_activation_quantiles")) return rc;
    hipLaunchKernelGGL(k_act_pick, dim3(2 * Q), dim3(ACT_THREADS), 0, s, sel, part, blocks, order);
    return pk_launch_status("pk_activation_quantiles");
}
