// Per-tensor statistics of a flat fp32 buffer (the optimiser's gradients, masters, moments, EMA): one 64-byte record per tensor of a
// segment table -- sums of x, x^2, |x| in fp64, min, max, and the counts of participating, inf/NaN and small elements -- in two launches
// for the whole model, and the latch that keeps the records of the last step that held a non-finite gradient.
//   k_tensor_stats_partial:  one WAVE per plan item (a chunk of <= TS_CHUNK elements of one tensor), four items per workgroup.  A tensor
//                            of <= 256 elements is one float4 per lane of one wave; the largest ones are spread over count / TS_CHUNK waves.
//   k_tensor_stats_finalize: one wave per tensor over its items' partial records.
//   k_tensor_stats_latch:    one workgroup over the final records.
// No atomics, no last-arriver.  Order of every sum: inside an item, lane l takes the item's float4 l, l + 64, ... and, if l < count % 4,
// tail element l last; the 64 lanes combine in the xor butterfly 32, 16, ..., 1; the finalize lane l takes partials l, l + 64, ... of its
// tensor and the same butterfly follows.  The plan fixes all of it: it does not depend on the grid, the stream or on capture.
#include "pk_common.h"

#include <math.h>

#define TS_CHUNK 2048           // elements per item: 8 float4 per lane
#define TS_MAX_ITEMS (1 << 24)  // 64-byte partials: the workspace stays below 2^31 bytes, and every index fits an int

struct __attribute__((aligned(16))) TsRecord {
    double sum, sumsq, sumabs;
    float mn, mx;
    int64_t n, nonfinite, small, zero;
};
static_assert(sizeof(TsRecord) == PK_TENSOR_STATS_RECORD_BYTES, "record layout");
// plan rows, 16 bytes each: n_tensors tensor rows, then n_items item rows (item rows of one tensor are consecutive, in chunk order)
struct __attribute__((aligned(16))) TsTensorRow { int32_t first_item, n_items; int64_t zero; };
struct __attribute__((aligned(16))) TsItemRow { int64_t start; int32_t count, tensor; };
static_assert(sizeof(TsTensorRow) == 16 && sizeof(TsItemRow) == 16, "plan layout");

struct TsAcc {
    double sum, sumsq, sumabs;
    float mn, mx;
    uint32_t n, nonfinite, small;
};

__device__ __forceinline__ void ts_take(TsAcc& c, float x, uint32_t flag, float tiny) {
    if (!(flag & 2u)) return;  // bit1: the element takes part in optimisation
    c.n += 1;
    if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {  // exponent bits all ones: inf / NaN (k_grad_sumsq's test)
        c.nonfinite += 1;
        return;
    }
    const double d = (double)x;
    c.sum += d;
    c.sumsq += d * d;  // exact in fp64, also for +-FLT_MAX
    c.sumabs += fabs(d);
    c.mn = fminf(c.mn, x);
    c.mx = fmaxf(c.mx, x);
    c.small += fabsf(x) <= tiny;
}

template <class V>
__device__ __forceinline__ V ts_wave_sum(V v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool DIFF, bool FLAGS>
__device__ __forceinline__ void ts_item(const float* __restrict__ a, const float* __restrict__ b, const uint8_t* __restrict__ flags,
                                        const TsItemRow it, float tiny, int lane, TsRecord* __restrict__ out) {
    TsAcc c = {0.0, 0.0, 0.0, INFINITY, -INFINITY, 0u, 0u, 0u};
    const float4* a4 = reinterpret_cast<const float4*>(a + it.start);
    const float4* b4 = reinterpret_cast<const float4*>(DIFF ? b + it.start : a);
    const uint32_t* f4 = reinterpret_cast<const uint32_t*>(FLAGS ? flags + it.start : nullptr);
    const int n4 = it.count >> 2;
    for (int base = 0; base < n4; base += 256) {  // four 16-byte loads per lane in flight
        float4 A[4], B[4];
        uint32_t F[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = base + 64 * u + lane;
            if (k < n4) {
                A[u] = a4[k];
                if constexpr (DIFF) B[u] = b4[k];
                F[u] = FLAGS ? f4[k] : 0x02020202u;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (base + 64 * u + lane < n4) {
                if constexpr (DIFF) {
                    A[u].x -= B[u].x;
                    A[u].y -= B[u].y;
                    A[u].z -= B[u].z;
                    A[u].w -= B[u].w;
                }
                ts_take(c, A[u].x, F[u], tiny);
                ts_take(c, A[u].y, F[u] >> 8, tiny);
                ts_take(c, A[u].z, F[u] >> 16, tiny);
                ts_take(c, A[u].w, F[u] >> 24, tiny);
            }
        }
    }
    if (lane < (it.count & 3)) {  // the tensor's last 1..3 elements: scalar loads, the padding behind them is never read
        const int64_t e = it.start + 4 * (int64_t)n4 + lane;
        float x = a[e];
        if constexpr (DIFF) x -= b[e];
        ts_take(c, x, FLAGS ? flags[e] : 2u, tiny);
    }
    c.sum = ts_wave_sum(c.sum);
    c.sumsq = ts_wave_sum(c.sumsq);
    c.sumabs = ts_wave_sum(c.sumabs);
    c.n = ts_wave_sum(c.n);
    c.nonfinite = ts_wave_sum(c.nonfinite);
    c.small = ts_wave_sum(c.small);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c.mn = fminf(c.mn, __shfl_xor(c.mn, o, 64));
        c.mx = fmaxf(c.mx, __shfl_xor(c.mx, o, 64));
    }
    if (lane == 0) {
        TsRecord r;
        r.sum = c.sum;
        r.sumsq = c.sumsq;
        r.sumabs = c.sumabs;
        r.mn = c.mn;
        r.mx = c.mx;
        r.n = c.n;
        r.nonfinite = c.nonfinite;
        r.small = c.small;
        r.zero = 0;
        *out = r;
    }
}

template <bool DIFF, bool FLAGS>
__global__ void __launch_bounds__(256) k_tensor_stats_partial(const float* __restrict__ a, const float* __restrict__ b,
                                                              const uint8_t* __restrict__ flags, const TsItemRow* __restrict__ items,
                                                              int n_items, float tiny, TsRecord* __restrict__ partials) {
    const int item = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);  // wave-uniform
    if (item >= n_items) return;                                     // whole waves leave; no barrier follows
    ts_item<DIFF, FLAGS>(a, b, flags, items[item], tiny, threadIdx.x & 63, partials + item);
}

__global__ void __launch_bounds__(256) k_tensor_stats_finalize(const TsTensorRow* __restrict__ rows, int n_tensors,
                                                               const TsRecord* __restrict__ partials, TsRecord* __restrict__ records) {
    const int t = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= n_tensors) return;
    const TsTensorRow row = rows[t];
    TsRecord r = {0.0, 0.0, 0.0, INFINITY, -INFINITY, 0, 0, 0, 0};
    for (int k = lane; k < row.n_items; k += 64) {
        const TsRecord p = partials[row.first_item + k];
        r.sum += p.sum;
        r.sumsq += p.sumsq;
        r.sumabs += p.sumabs;
        r.mn = fminf(r.mn, p.mn);
        r.mx = fmaxf(r.mx, p.mx);
        r.n += p.n;
        r.nonfinite += p.nonfinite;
        r.small += p.small;
    }
    r.sum = ts_wave_sum(r.sum);
    r.sumsq = ts_wave_sum(r.sumsq);
    r.sumabs = ts_wave_sum(r.sumabs);
    r.n = ts_wave_sum((long long)r.n);
    r.nonfinite = ts_wave_sum((long long)r.nonfinite);
    r.small = ts_wave_sum((long long)r.small);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        r.mn = fminf(r.mn, __shfl_xor(r.mn, o, 64));
        r.mx = fmaxf(r.mx, __shfl_xor(r.mx, o, 64));
    }
    if (lane == 0) records[t] = r;
}

// The one decision taken on the device: a replayed graph has no host that could look at the records between steps.  latch_state:
// [0] events, [1] first offending tensor, [2] last offending tensor, [3] offending tensors, of the latest event.  Nothing is written
// when every record is clean.
__global__ void __launch_bounds__(256) k_tensor_stats_latch(const TsRecord* __restrict__ records, int n_tensors,
                                                            TsRecord* __restrict__ latched, int32_t* __restrict__ latch_state) {
    __shared__ int red[4];
    int first = 0x7fffffff, last = -1, bad = 0;
    for (int t = threadIdx.x; t < n_tensors; t += 256) {
        if (records[t].nonfinite > 0) {
            first = first < t ? first : t;
            last = t;
            bad += 1;
        }
    }
    bad = block_reduce<4>(bad, red, SumOp());
    if (bad == 0) return;  // uniform over the workgroup
    first = block_reduce<4>(first, red, MinOp());
    last = block_reduce<4>(last, red, MaxOp());
    const uint4* src = reinterpret_cast<const uint4*>(records);
    uint4* dst = reinterpret_cast<uint4*>(latched);
    for (int64_t i = threadIdx.x; i < (int64_t)n_tensors * 4; i += 256) dst[i] = src[i];
    if (threadIdx.x == 0) {
        latch_state[0] += 1;
        latch_state[1] = first;
        latch_state[2] = last;
        latch_state[3] = bad;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
extern "C" int pk_tensor_stats_chunk_elems(void) { return TS_CHUNK; }

extern "C" int pk_tensor_stats_plan_bytes(int n_items, int n_tensors) {
    PK_REQUIRE(n_tensors > 0 && n_items >= n_tensors && n_items <= TS_MAX_ITEMS,
               "pk_tensor_stats_plan_bytes: n_items=%d n_tensors=%d: need 1 <= n_tensors <= n_items <= %d", n_items, n_tensors,
               TS_MAX_ITEMS);
    return (int)(sizeof(TsTensorRow) * (size_t)n_tensors + sizeof(TsItemRow) * (size_t)n_items);
}

extern "C" int pk_tensor_stats_ws_bytes(int n_items, int n_tensors) {
    PK_REQUIRE(n_tensors > 0 && n_items >= n_tensors && n_items <= TS_MAX_ITEMS,
               "pk_tensor_stats_ws_bytes: n_items=%d n_tensors=%d: need 1 <= n_tensors <= n_items <= %d", n_items, n_tensors, TS_MAX_ITEMS);
    return (int)(sizeof(TsRecord) * (size_t)n_items);
}

extern "C" int pk_tensor_stats_plan(const int64_t* seg_host, int n_tensors, void* plan_out_host, int64_t capacity_bytes) {
    PK_REQUIRE(seg_host, "pk_tensor_stats_plan: null segment table");
    PK_REQUIRE(n_tensors > 0, "pk_tensor_stats_plan: n_tensors=%d must be positive", n_tensors);
    int64_t n_items = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const int64_t off = seg_host[2 * t], cnt = seg_host[2 * t + 1];
        PK_REQUIRE(off >= 0 && (off & 3) == 0, "pk_tensor_stats_plan: tensor %d: offset %lld must be a non-negative multiple of 4", t,
                   (long long)off);
        PK_REQUIRE(cnt >= 1 && cnt <= ((int64_t)1 << 40), "pk_tensor_stats_plan: tensor %d: count %lld outside [1, 2^40]", t,
                   (long long)cnt);
        n_items += (cnt + TS_CHUNK - 1) / TS_CHUNK;
        PK_REQUIRE(n_items <= TS_MAX_ITEMS, "pk_tensor_stats_plan: more than %d items", TS_MAX_ITEMS);
    }
    if (!plan_out_host) return (int)n_items;
    const int64_t need = (int64_t)sizeof(TsTensorRow) * n_tensors + (int64_t)sizeof(TsItemRow) * n_items;
    PK_REQUIRE(capacity_bytes >= need, "pk_tensor_stats_plan: the plan needs %lld bytes (pk_tensor_stats_plan_bytes), capacity is %lld",
               (long long)need, (long long)capacity_bytes);
    PK_REQUIRE(((uintptr_t)plan_out_host & 7) == 0, "pk_tensor_stats_plan: plan_out_host must be 8-byte aligned");
    // written through plain words: the host buffer only has to be 8-byte aligned
    int64_t* w = reinterpret_cast<int64_t*>(plan_out_host);
    int32_t* w32 = reinterpret_cast<int32_t*>(plan_out_host);
    int64_t item = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const int64_t off = seg_host[2 * t], cnt = seg_host[2 * t + 1];
        const int64_t chunks = (cnt + TS_CHUNK - 1) / TS_CHUNK;
        w32[4 * t] = (int32_t)item;
        w32[4 * t + 1] = (int32_t)chunks;
        w[2 * t + 1] = 0;
        for (int64_t c = 0; c < chunks; ++c, ++item) {
            const int64_t row = n_tensors + item, left = cnt - c * TS_CHUNK;
            w[2 * row] = off + c * TS_CHUNK;
            w32[4 * row + 2] = (int32_t)(left < TS_CHUNK ? left : TS_CHUNK);
            w32[4 * row + 3] = t;
        }
    }
    return (int)n_items;
}

extern "C" int pk_tensor_stats(const float* a, const float* b, const uint8_t* flags, const void* plan_dev, int n_tensors, int n_items,
                               float tiny, void* ws, int64_t ws_bytes, void* records, void* stream) {
    PK_REQUIRE(a && plan_dev && ws && records, "pk_tensor_stats: null pointer");
    PK_REQUIRE(n_tensors > 0 && n_items >= n_tensors && n_items <= TS_MAX_ITEMS,
               "pk_tensor_stats: n_items=%d n_tensors=%d: need 1 <= n_tensors <= n_items <= %d", n_items, n_tensors, TS_MAX_ITEMS);
    PK_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)plan_dev | (uintptr_t)ws | (uintptr_t)records) & 15) == 0 &&
                   ((uintptr_t)flags & 3) == 0,
               "pk_tensor_stats: misaligned buffer (a, b, plan, ws, records: 16 bytes; flags: 4)");
    PK_REQUIRE(tiny >= 0.f && isfinite(tiny), "pk_tensor_stats: tiny=%g must be finite and >= 0", (double)tiny);  // false for NaN too
    PK_REQUIRE(ws_bytes >= (int64_t)sizeof(TsRecord) * n_items, "pk_tensor_stats: ws_bytes=%lld, but %d items need %lld (pk_tensor_stats_ws_bytes)",
               (long long)ws_bytes, n_items, (long long)sizeof(TsRecord) * n_items);
    const TsTensorRow* rows = reinterpret_cast<const TsTensorRow*>(plan_dev);
    const TsItemRow* items = reinterpret_cast<const TsItemRow*>(rows + n_tensors);
    TsRecord* partials = reinterpret_cast<TsRecord*>(ws);
    const dim3 grid((unsigned)((n_items + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (b && flags)
        hipLaunchKernelGGL((k_tensor_stats_partial<true, true>), grid, block, 0, s, a, b, flags, items, n_items, tiny, partials);
    else if (b)
        hipLaunchKernelGGL((k_tensor_stats_partial<true, false>), grid, block, 0, s, a, b, flags, items, n_items, tiny, partials);
    else if (flags)
        hipLaunchKernelGGL((k_tensor_stats_partial<false, true>), grid, block, 0, s, a, b, flags, items, n_items, tiny, partials);
    else
        hipLaunchKernelGGL((k_tensor_stats_partial<false, false>), grid, block, 0, s, a, b, flags, items, n_items, tiny, partials);
    if (int rc = pk_launch_status("pk_tensor_stats")) return rc;
    hipLaunchKernelGGL(k_tensor_stats_finalize, dim3((unsigned)((n_tensors + 3) / 4)), block, 0, s, rows, n_tensors, partials,
                       reinterpret_cast<TsRecord*>(records));
    return pk_launch_status("pk_tensor_stats");
}

extern "C" int pk_tensor_stats_latch(const void* records, int n_tensors, void* latched, int32_t* latch_state, void* stream) {
    PK_REQUIRE(records && latched && latch_state, "pk_tensor_stats_latch: null pointer");
    PK_REQUIRE(n_tensors > 0 && n_tensors <= TS_MAX_ITEMS, "pk_tensor_stats_latch: n_tensors=%d outside [1, %d]", n_tensors, TS_MAX_ITEMS);
    PK_REQUIRE((((uintptr_t)records | (uintptr_t)latched) & 15) == 0 && ((uintptr_t)latch_state & 3) == 0,
               "pk_tensor_stats_latch: misaligned buffer (records, latched: 16 bytes; latch_state: 4)");
    PK_REQUIRE(records != latched, "pk_tensor_stats_latch: latched must be a buffer of its own");
    hipLaunchKernelGGL(k_tensor_stats_latch, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const TsRecord*>(records),
                       n_tensors, reinterpret_cast<TsRecord*>(latched), latch_state);
    return pk_launch_status("pk_tensor_stats_latch");
}
