// Localisation error analysis (this project's own specification: DESIGN.md "Localisation error analysis").  The reference's
// PerformanceAnalyzer (analysis/nn_quantitative_viz.py:105-252) loops over every prediction in Python three times: the per-joint error
// lists behind its box and violin plots, the calibration curve over confidence bins, and precision / recall over a confidence threshold.
// Two entries, each one launch:
//   pk_kpt_error             one 256-thread workgroup per joint, threads stride over the samples: the error of every pair into a (K, ld)
//                            store, calibration and precision / recall counts into int32 LDS histograms, then int64 global counters
//   pk_kpt_error_quantiles   one workgroup per (joint, quantile): exact order statistics of a row of the store by radix select
// No float atomics and no global atomics.  The counters are integers (LDS atomicAdd: order-free), the order statistics are exact, and the
// one floating-point sum is taken in a fixed order (per thread in ascending column, then `block_reduce`): the same input gives the same bits.
#include "pk_common.h"

#define ERR_THREADS 256                                           // MOTION_THREADS of pk_motion.hip: the analysis units' workgroup
#define ERR_WAVES (ERR_THREADS / PK_WAVE)

// ================================================================================================ errors, calibration, precision / recall
// Pair (n, k) counts iff vis > 0, the four coordinates are finite and (norm == NULL or norm[n] > 0): pk_pck's rule.  float32, one rounding
// per operation (-ffp-contract=off: no FMA): dx = px - gx, dy = py - gy, d2 = dx dx + dy dy; e = (float)sqrt((double)d2) and, with norm,
// e = (float)((double)e / (double)norm[n]): float64 then narrow equals the correctly rounded float32 operation, however sqrtf or / are
// lowered.  hit = e < pixel_thr.  An uncounted pair stores NaN and touches no counter.
__global__ void __launch_bounds__(ERR_THREADS) k_kpt_error(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const float* __restrict__ vis, const float* __restrict__ conf,
                                                           const float* __restrict__ norm, float pixel_thr,
                                                           const float* __restrict__ bin_edges, int n_bins,
                                                           const float* __restrict__ conf_thr, int T, float* __restrict__ err_out, int64_t ld,
                                                           int64_t* __restrict__ calib_count, int64_t* __restrict__ calib_hit,
                                                           int64_t* __restrict__ pr_hist, int N, int K) {
    __shared__ int s_count[PK_ERR_MAX_BINS], s_hit[PK_ERR_MAX_BINS], s_pr[2 * (PK_ERR_MAX_CONF_THR + 1)];
    __shared__ float s_edges[PK_ERR_MAX_BINS + 1], s_thr[PK_ERR_MAX_CONF_THR];      // the two searches run on LDS copies of the tables
    const int k = blockIdx.x, n_pr = 2 * (T + 1);
    if (conf != nullptr) {                                        // uniform over the block
        for (int i = threadIdx.x; i < n_bins; i += ERR_THREADS) s_count[i] = s_hit[i] = 0;
        for (int i = threadIdx.x; i < n_pr; i += ERR_THREADS) s_pr[i] = 0;
        for (int i = threadIdx.x; i <= n_bins; i += ERR_THREADS) s_edges[i] = bin_edges[i];
        for (int i = threadIdx.x; i < T; i += ERR_THREADS) s_thr[i] = conf_thr[i];
        __syncthreads();
    }
    float* __restrict__ row = err_out + (size_t)k * ld;
    for (int64_t n = threadIdx.x; n < N; n += ERR_THREADS) {      // 64-bit: n + 256 may pass 2^31
        const size_t i = (size_t)n * K + k;
        const float px = pred[2 * i], py = pred[2 * i + 1], gx = gt[2 * i], gy = gt[2 * i + 1];
        const float nm = norm != nullptr ? norm[n] : 1.f;
        if (!(vis[i] > 0.f && nm > 0.f && isfinite(px) && isfinite(py) && isfinite(gx) && isfinite(gy))) {
            row[n] = __builtin_nanf("");
            continue;
        }
        const float dx = px - gx, dy = py - gy;
        const float d2 = dx * dx + dy * dy;
        float e = (float)sqrt((double)d2);
        if (norm != nullptr) e = (float)((double)e / (double)nm);
        row[n] = e;
        if (conf == nullptr) continue;
        const float c = conf[i];
        if (!isfinite(c)) continue;                               // stays in the store, enters neither calibration nor precision / recall
        const int hit = e < pixel_thr ? 1 : 0;
        // calibration: bin b takes edges[b] <= c < edges[b + 1]; j = number of edges <= c (ascending edges: binary search), b = j - 1
        int lo = 0, hi = n_bins + 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_edges[mid] <= c) lo = mid + 1; else hi = mid;
        }
        if (lo >= 1 && lo <= n_bins) {
            atomicAdd(&s_count[lo - 1], 1);                       // integer counts in LDS: order-free
            if (hit) atomicAdd(&s_hit[lo - 1], 1);
        }
        // precision / recall: m = number of thresholds with c > t (ascending thresholds), 0 <= m <= T
        int a = 0, b = T;
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (s_thr[mid] < c) a = mid + 1; else b = mid;
        }
        atomicAdd(&s_pr[(hit ? 0 : T + 1) + a], 1);
    }
    if (conf == nullptr) return;
    __syncthreads();
    // one workgroup owns joint k and launches on one stream are ordered: one writer per counter, plain read-add-write
    for (int i = threadIdx.x; i < n_bins; i += ERR_THREADS) {
        calib_count[(size_t)k * n_bins + i] += s_count[i];
        calib_hit[(size_t)k * n_bins + i] += s_hit[i];
    }
    for (int i = threadIdx.x; i < n_pr; i += ERR_THREADS) pr_hist[(size_t)k * n_pr + i] += s_pr[i];
}

extern "C" int pk_kpt_error(const float* pred, const float* gt, const float* vis, const float* conf, const float* norm, float pixel_thr,
                            const float* bin_edges, int n_bins, const float* conf_thr, int T, float* err_out, int64_t ld,
                            int64_t* calib_count, int64_t* calib_hit, int64_t* pr_hist, int N, int K, void* stream) {
    PK_REQUIRE(pred && gt && vis && err_out, "pk_kpt_error: null pointer");
    PK_REQUIRE(!conf || (bin_edges && conf_thr && calib_count && calib_hit && pr_hist),
               "pk_kpt_error: null pointer (a confidence needs bin_edges, conf_thr and the three counters)");
    PK_REQUIRE(N > 0 && K > 0, "pk_kpt_error: bad shape N=%d K=%d", N, K);
    PK_REQUIRE(ld >= N, "pk_kpt_error: row stride ld=%lld below N=%d", (long long)ld, N);
    if (conf) {
        PK_REQUIRE(n_bins >= 1 && n_bins <= PK_ERR_MAX_BINS, "pk_kpt_error: %d confidence bins (1 to %d)", n_bins, PK_ERR_MAX_BINS);
        PK_REQUIRE(T >= 1 && T <= PK_ERR_MAX_CONF_THR, "pk_kpt_error: %d confidence thresholds (1 to %d)", T, PK_ERR_MAX_CONF_THR);
    }
    hipLaunchKernelGGL(k_kpt_error, dim3(K), dim3(ERR_THREADS), 0, (hipStream_t)stream, pred, gt, vis, conf, norm, pixel_thr, bin_edges, n_bins,
                       conf_thr, T, err_out, ld, calib_count, calib_hit, pr_hist, N, K);
    return pk_launch_status("pk_kpt_error");
}

// ================================================================================================ exact order statistics of the store
// Inclusive scan of the 256-bin histogram (thread t owns bin t) and the bin that holds rank r: the one with excl <= r < incl.  Returns the
// bin in pick[0], the number of elements in lower bins in pick[1] and the bin's own count in pick[2] to every thread.  Integers: exact.
__device__ __forceinline__ void pick_bin(const int* hist, int* wave_sum, int* pick, int r) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int h = hist[threadIdx.x];
    int inc = h;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    for (int i = 0; i < w; ++i) inc += wave_sum[i];
    const int excl = inc - h;
    if (excl <= r && r < inc) pick[0] = threadIdx.x, pick[1] = excl, pick[2] = h;
    __syncthreads();
}

// Row k of the store, NaN entries left out: n values v[0] <= ... <= v[n-1], all non-negative (errors), so that the unsigned bit pattern
// orders them.  pos = q (double)(n - 1), lo = floor(pos), hi = min(lo + 1, n - 1).  v[lo] by radix select: four 8-bit passes from the top
// byte, each a 256-bin LDS histogram of the elements that match the prefix found so far.  The select also gives the number of elements
// <= v[lo]; hi below it: v[hi] = v[lo]; otherwise v[hi] is the minimum over the elements with a larger key.
__global__ void __launch_bounds__(ERR_THREADS) k_kpt_error_quantiles(const float* __restrict__ err, int64_t ld, int64_t n_cols,
                                                                     const double* __restrict__ q, int Q, float* __restrict__ order,
                                                                     double* __restrict__ summary) {
    __shared__ int hist[256], wave_sum[ERR_WAVES], pick[3], red_i[ERR_WAVES];
    __shared__ float red_f[ERR_WAVES];
    __shared__ double red_d[ERR_WAVES];
    const int k = blockIdx.x, qi = blockIdx.y;
    const float* __restrict__ row = err + (size_t)k * ld;
    float* o = order + ((size_t)k * Q + qi) * 2;

    int cnt = 0;
    if (qi == 0) {                                                // uniform over the block: these workgroups also write the summary
        double sum = 0.0;
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
        for (int64_t i = threadIdx.x; i < n_cols; i += ERR_THREADS) {
            const float v = row[i];
            if (v != v) continue;
            ++cnt;
            sum += (double)v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        const double ts = block_reduce<ERR_WAVES>(sum, red_d, SumOp());
        const float lo_v = block_reduce<ERR_WAVES>(mn, red_f, MinOp()), hi_v = block_reduce<ERR_WAVES>(mx, red_f, MaxOp());
        const int tn = block_reduce<ERR_WAVES>(cnt, red_i, SumOp());
        if (threadIdx.x == 0) {
            double* s = summary + (size_t)k * 4;
            s[0] = (double)tn;
            s[1] = tn ? ts : 0.0;
            s[2] = tn ? (double)lo_v : 0.0;
            s[3] = tn ? (double)hi_v : 0.0;
        }
        cnt = tn;
    } else {
#pragma unroll 4
        for (int64_t i = threadIdx.x; i < n_cols; i += ERR_THREADS) {
            const float v = row[i];
            cnt += v == v ? 1 : 0;
        }
        cnt = block_reduce<ERR_WAVES>(cnt, red_i, SumOp());
    }
    const int n = cnt;                                            // n_cols <= 2^31 - 1: fits
    if (n == 0) {
        if (threadIdx.x == 0) o[0] = o[1] = 0.f;
        return;
    }
    const double pos = q[qi] * (double)(n - 1);
    const int lo = pos >= 0.0 ? (pos < (double)(n - 1) ? (int)floor(pos) : n - 1) : 0;      // q outside [0, 1] or NaN: clamped, never out of range
    const int hi = lo + 1 < n ? lo + 1 : n - 1;

    uint32_t prefix = 0;
    int r = lo, below = 0, equal = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll 4
        for (int64_t i = threadIdx.x; i < n_cols; i += ERR_THREADS) {
            const float v = row[i];
            const uint32_t b = __float_as_uint(v);
            if (v == v && (shift == 24 || (b >> (shift + 8)) == prefix)) atomicAdd(&hist[(b >> shift) & 255u], 1);
        }
        __syncthreads();
        pick_bin(hist, wave_sum, pick, r);
        prefix = (prefix << 8) | (uint32_t)pick[0];
        r -= pick[1];
        below += pick[1];
        equal = pick[2];
        __syncthreads();                                          // pick and hist are rewritten by the next pass
    }
    const float v_lo = __uint_as_float(prefix);
    float v_hi = v_lo;
    if (hi >= below + equal) {                                    // uniform over the block; then an element with a larger key exists
        float mn = INFINITY;
#pragma unroll 4
        for (int64_t i = threadIdx.x; i < n_cols; i += ERR_THREADS) {
            const float v = row[i];
            if (v == v && __float_as_uint(v) > prefix) mn = v < mn ? v : mn;
        }
        v_hi = block_reduce<ERR_WAVES>(mn, red_f, MinOp());
    }
    if (threadIdx.x == 0) o[0] = v_lo, o[1] = v_hi;
}

extern "C" int pk_kpt_error_quantiles(const float* err, int64_t ld, int64_t n_cols, int K, const double* q, int Q, float* order,
                                      double* summary, void* stream) {
    PK_REQUIRE(err && q && order && summary, "pk_kpt_error_quantiles: null pointer");
    PK_REQUIRE(Q >= 1 && Q <= PK_ERR_MAX_QUANTILES, "pk_kpt_error_quantiles: %d quantiles (1 to %d)", Q, PK_ERR_MAX_QUANTILES);
    PK_REQUIRE(K > 0 && n_cols > 0 && n_cols <= PK_ERR_MAX_COLS, "pk_kpt_error_quantiles: bad shape K=%d n_cols=%lld (1 to %d columns)", K,
               (long long)n_cols, PK_ERR_MAX_COLS);
    PK_REQUIRE(ld >= n_cols, "pk_kpt_error_quantiles: row stride ld=%lld below n_cols=%lld", (long long)ld, (long long)n_cols);
    hipLaunchKernelGGL(k_kpt_error_quantiles, dim3(K, Q), dim3(ERR_THREADS), 0, (hipStream_t)stream, err, ld, n_cols, q, Q, order, summary);
    return pk_launch_status("pk_kpt_error_quantiles");
}
