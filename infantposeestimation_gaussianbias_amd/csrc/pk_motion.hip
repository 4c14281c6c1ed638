// Movement analysis and PCK on pose sequences (this project's own specification: DESIGN.md "Movement analysis and PCK").  The reference
// imports calculate_movement_amplitude / calculate_temporal_consistency from utils.metrics (examples/quick_start.py:159,
// visualization.py:385,441) and asks for PCK in both yamls, and defines none of the three; plot_movement_heatmap (visualization.py:230) bins
// joint positions with np.histogram2d.  Three entries, each one launch:
//   pk_pck                  one 256-thread workgroup per joint, threads stride over the samples
//   pk_motion_stats         one workgroup per (sequence, joint), threads stride over the frames
//   pk_position_histogram   one workgroup per (sequence, joint), int32 histogram in LDS
// and, at the end, the reference's own post-processing of pose sequences: pk_temporal_smooth and pk_nms_pose.
// No float atomics.  Every floating-point sum is taken in a fixed order (per thread in ascending index, then the xor butterfly inside the
// wave, then the waves in order), so two runs give identical bits; counts, minima and maxima are exact in any order.
#include "pk_common.h"

#define MOTION_THREADS 256
#define MOTION_WAVES (MOTION_THREADS / PK_WAVE)

__device__ __forceinline__ bool finite2(float x, float y) { return isfinite(x) && isfinite(y); }

// ================================================================================================ PCK
// Pair (n, k) counts iff vis > 0, norm[n] > 0 and the four coordinates are finite.  The decision is float32, one rounding per operation
// (-ffp-contract=off: no FMA), without a square root: dx = px - gx, dy = py - gy, d2 = dx dx + dy dy, r = thr norm, hit iff d2 <= r r.
// err_sum adds sqrt((double)d2) / (double)norm.  The three outputs accumulate over launches (one workgroup owns joint k, launches on one
// stream are ordered: plain read-add-write).
__global__ void __launch_bounds__(MOTION_THREADS) k_pck(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ vis,
                                                        const float* __restrict__ norm, const float* __restrict__ thresholds,
                                                        int64_t* __restrict__ correct, int64_t* __restrict__ valid, double* __restrict__ err_sum,
                                                        int N, int K, int n_thr) {
    __shared__ double red_d[MOTION_WAVES];
    __shared__ int red_i[MOTION_WAVES];
    const int k = blockIdx.x;
    float thr[PK_PCK_MAX_THR];
    int hit[PK_PCK_MAX_THR];
#pragma unroll
    for (int j = 0; j < PK_PCK_MAX_THR; ++j) {
        thr[j] = j < n_thr ? thresholds[j] : 0.f;
        hit[j] = 0;
    }
    int n_valid = 0;
    double err = 0.0;
    for (int n = threadIdx.x; n < N; n += MOTION_THREADS) {
        const size_t i = (size_t)n * K + k;
        const float px = pred[2 * i], py = pred[2 * i + 1], gx = gt[2 * i], gy = gt[2 * i + 1], nm = norm[n];
        if (!(vis[i] > 0.f && nm > 0.f && finite2(px, py) && finite2(gx, gy))) continue;
        const float dx = px - gx, dy = py - gy;
        const float d2 = dx * dx + dy * dy;
        ++n_valid;
        err += sqrt((double)d2) / (double)nm;
#pragma unroll
        for (int j = 0; j < PK_PCK_MAX_THR; ++j) {
            const float r = thr[j] * nm;
            hit[j] += (j < n_thr && d2 <= r * r) ? 1 : 0;
        }
    }
    const int tv = block_reduce<MOTION_WAVES>(n_valid, red_i, SumOp());
    const double te = block_reduce<MOTION_WAVES>(err, red_d, SumOp());
    if (threadIdx.x == 0) {
        valid[k] += tv;
        err_sum[k] += te;
    }
#pragma unroll
    for (int j = 0; j < PK_PCK_MAX_THR; ++j) {
        if (j < n_thr) {                                          // uniform over the block
            const int th = block_reduce<MOTION_WAVES>(hit[j], red_i, SumOp());
            if (threadIdx.x == 0) correct[(size_t)j * K + k] += th;
        }
    }
}

extern "C" int pk_pck(const float* pred, const float* gt, const float* vis, const float* norm, const float* thresholds, int64_t* correct,
                      int64_t* valid, double* err_sum, int N, int K, int n_thr, void* stream) {
    PK_REQUIRE(pred && gt && vis && norm && thresholds && correct && valid && err_sum, "pk_pck: null pointer");
    PK_REQUIRE(N > 0 && K > 0, "pk_pck: bad shape N=%d K=%d", N, K);
    PK_REQUIRE(n_thr >= 1 && n_thr <= PK_PCK_MAX_THR, "pk_pck: %d thresholds (1 to %d)", n_thr, PK_PCK_MAX_THR);
    hipLaunchKernelGGL(k_pck, dim3(K), dim3(MOTION_THREADS), 0, (hipStream_t)stream, pred, gt, vis, norm, thresholds, correct, valid, err_sum,
                       N, K, n_thr);
    return pk_launch_status("pk_pck");
}

// ================================================================================================ per-joint movement statistics
// Frame t of joint k is valid by `seq_frame`'s rule (pk_common.h), a frame outside [0, T) is not.  A step t -> t+1 counts iff both
// frames are valid, a triple iff t-1, t, t+1 are.  The thread that owns frame t takes the step that starts at t and the triple centred on
// t.  Differences, norms (sqrt(dx dx + dy dy), no FMA) and sums in float64; the float32 inputs widen exactly.
__device__ __forceinline__ SeqFrame motion_frame(const float* __restrict__ coords, const float* __restrict__ conf, size_t base, int K, int t, int T,
                                                 float min_conf) {
    if (t < 0 || t >= T) return SeqFrame{0.0, 0.0, false};
    return seq_frame(coords, conf, base, K, t, min_conf);
}

__global__ void __launch_bounds__(MOTION_THREADS) k_motion_stats(const float* __restrict__ coords, const float* __restrict__ conf,
                                                                 double* __restrict__ stats, int T, int K, float min_conf) {
    __shared__ double red_d[MOTION_WAVES];
    __shared__ float red_f[MOTION_WAVES];
    __shared__ int red_i[MOTION_WAVES];
    const int s = blockIdx.x / K, k = blockIdx.x - s * K;
    const size_t base = (size_t)s * T * K + k;                    // frame t of this joint: element base + t K of (S,T,K)
    int n_valid = 0, n_steps = 0, n_triples = 0;
    float min_x = INFINITY, max_x = -INFINITY, min_y = INFINITY, max_y = -INFINITY;
    double path = 0.0, max_step = 0.0, accel = 0.0;
    for (int t = threadIdx.x; t < T; t += MOTION_THREADS) {
        const SeqFrame c = motion_frame(coords, conf, base, K, t, T, min_conf);
        if (!c.ok) continue;
        const float cx = (float)c.x, cy = (float)c.y;
        ++n_valid;
        min_x = fminf(min_x, cx), max_x = fmaxf(max_x, cx), min_y = fminf(min_y, cy), max_y = fmaxf(max_y, cy);
        const SeqFrame nx = motion_frame(coords, conf, base, K, t + 1, T, min_conf);
        if (!nx.ok) continue;
        const double dx = nx.x - c.x, dy = nx.y - c.y;
        const double step = sqrt(dx * dx + dy * dy);
        ++n_steps;
        path += step;
        max_step = step > max_step ? step : max_step;
        const SeqFrame pv = motion_frame(coords, conf, base, K, t - 1, T, min_conf);
        if (!pv.ok) continue;
        const double ax = (nx.x - 2.0 * c.x) + pv.x, ay = (nx.y - 2.0 * c.y) + pv.y;
        ++n_triples;
        accel += sqrt(ax * ax + ay * ay);
    }
    const int tv = block_reduce<MOTION_WAVES>(n_valid, red_i, SumOp()), ts = block_reduce<MOTION_WAVES>(n_steps, red_i, SumOp()),
              tt = block_reduce<MOTION_WAVES>(n_triples, red_i, SumOp());
    const float lo_x = block_reduce<MOTION_WAVES>(min_x, red_f, MinOp()), hi_x = block_reduce<MOTION_WAVES>(max_x, red_f, MaxOp()),
                lo_y = block_reduce<MOTION_WAVES>(min_y, red_f, MinOp()), hi_y = block_reduce<MOTION_WAVES>(max_y, red_f, MaxOp());
    const double tp = block_reduce<MOTION_WAVES>(path, red_d, SumOp()), tm = block_reduce<MOTION_WAVES>(max_step, red_d, MaxOp()),
                 ta = block_reduce<MOTION_WAVES>(accel, red_d, SumOp());
    if (threadIdx.x == 0) {
        double* o = stats + (size_t)blockIdx.x * 11;
        const double rx = tv ? (double)hi_x - (double)lo_x : 0.0, ry = tv ? (double)hi_y - (double)lo_y : 0.0;
        o[0] = (double)tv;
        o[1] = tv ? (double)lo_x : 0.0;
        o[2] = tv ? (double)hi_x : 0.0;
        o[3] = tv ? (double)lo_y : 0.0;
        o[4] = tv ? (double)hi_y : 0.0;
        o[5] = sqrt(rx * rx + ry * ry);
        o[6] = tp;
        o[7] = (double)ts;
        o[8] = tm;
        o[9] = ta;
        o[10] = (double)tt;
    }
}

extern "C" int pk_motion_stats(const float* coords, const float* conf, double* stats, int S, int T, int K, float min_conf, void* stream) {
    PK_REQUIRE(coords && stats, "pk_motion_stats: null pointer");
    if (const int rc = seq_shape_check("pk_motion_stats", S, T, K)) return rc;
    hipLaunchKernelGGL(k_motion_stats, dim3(S * K), dim3(MOTION_THREADS), 0, (hipStream_t)stream, coords, conf, stats, T, K, min_conf);
    return pk_launch_status("pk_motion_stats");
}

// ================================================================================================ position histogram
// np.histogram2d's rule for any ascending edges: bin i holds e[i] <= v < e[i+1], the last bin also v == e[nb]; anything outside
// [e[0], e[nb]] is dropped.  The bin is guessed in float64 from the end edges, clamped, and corrected by walking along the edges, which
// makes the result independent of how the guess rounds.  Returns -1 for a dropped value.
__device__ __forceinline__ int edge_bin(double v, const double* __restrict__ e, int nb) {
    if (!(v >= e[0] && v <= e[nb])) return -1;
    double g = floor((v - e[0]) / (e[nb] - e[0]) * (double)nb);
    g = g >= 0.0 ? g : 0.0;                                       // also catches NaN (e[0] == e[nb])
    int i = g < (double)(nb - 1) ? (int)g : nb - 1;
    while (i > 0 && v < e[i]) --i;
    while (i < nb - 1 && v >= e[i + 1]) ++i;
    return i;
}

__global__ void __launch_bounds__(MOTION_THREADS) k_position_histogram(const float* __restrict__ coords, const float* __restrict__ conf,
                                                                       const double* __restrict__ edges_x, const double* __restrict__ edges_y,
                                                                       int32_t* __restrict__ counts, int T, int K, int nbx, int nby,
                                                                       float min_conf) {
    extern __shared__ int hist[];
    const int s = blockIdx.x / K, k = blockIdx.x - s * K, nb = nbx * nby;
    const size_t base = (size_t)s * T * K + k;
    for (int i = threadIdx.x; i < nb; i += MOTION_THREADS) hist[i] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += MOTION_THREADS) {
        const SeqFrame c = motion_frame(coords, conf, base, K, t, T, min_conf);
        if (!c.ok) continue;
        const int bx = edge_bin(c.x, edges_x, nbx), by = edge_bin(c.y, edges_y, nby);
        if (bx >= 0 && by >= 0) atomicAdd(&hist[by * nbx + bx], 1);      // integer counts: order-free
    }
    __syncthreads();
    int32_t* o = counts + (size_t)blockIdx.x * nb;
    for (int i = threadIdx.x; i < nb; i += MOTION_THREADS) o[i] = hist[i];
}

extern "C" int pk_position_histogram(const float* coords, const float* conf, const double* edges_x, const double* edges_y, int32_t* counts,
                                     int S, int T, int K, int nbx, int nby, float min_conf, void* stream) {
    PK_REQUIRE(coords && edges_x && edges_y && counts, "pk_position_histogram: null pointer");
    if (const int rc = seq_shape_check("pk_position_histogram", S, T, K)) return rc;
    PK_REQUIRE(nbx > 0 && nby > 0, "pk_position_histogram: bad bin counts %d x %d", nbx, nby);
    PK_SUPPORTED((int64_t)nbx * nby <= PK_HIST_MAX_BINS,
                 "pk_position_histogram: %d x %d bins exceed the %d a workgroup keeps in LDS; take larger bins", nbx, nby, PK_HIST_MAX_BINS);
    hipLaunchKernelGGL(k_position_histogram, dim3(S * K), dim3(MOTION_THREADS), (size_t)nbx * nby * sizeof(int), (hipStream_t)stream, coords,
                       conf, edges_x, edges_y, counts, T, K, nbx, nby, min_conf);
    return pk_launch_status("pk_position_histogram");
}

// ================================================================================================ video post-processing
// utils/postprocess.py::temporal_smoothing (:187-223): per joint coordinate, edge-padded trajectory convolved (np.convolve,
// i.e. with the kernel FLIPPED) with `w` weights, evaluated in float64 and stored as float32 like the reference's
// numpy-float64 -> float32 tensor assignment.  coords/out: (T, C) with C = 2K; weights: w doubles; w must be odd (the
// reference's output has T+1 entries for even windows and its assignment fails).
__global__ void __launch_bounds__(256) k_temporal_smooth(const float* __restrict__ coords, float* __restrict__ out,
                                                         const double* __restrict__ weights, int T, int C, int w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * C) return;
    const int t = i / C, c = i - t * C, half = w / 2;
    double acc = 0.0;
    for (int j = 0; j < w; ++j) {
        int src = t + (w - 1 - j) - half;                 // padded index t + w-1-j, minus the left pad
        src = src < 0 ? 0 : (src >= T ? T - 1 : src);     // mode='edge'
        acc += (double)coords[(size_t)src * C + c] * weights[j];
    }
    out[i] = (float)acc;
}
extern "C" int pk_temporal_smooth(const float* coords, float* out, const double* weights, int T, int C, int window, void* stream) {
    PK_REQUIRE(coords && out && weights && T > 0 && C > 0 && window > 0, "pk_temporal_smooth: bad argument");
    PK_SUPPORTED((window & 1) == 1, "pk_temporal_smooth: window %d must be odd (the reference fails on even windows)", window);
    hipLaunchKernelGGL(k_temporal_smooth, dim3((T * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, coords, out, weights, T, C, window);
    return pk_launch_status("pk_temporal_smooth");
}

// utils/postprocess.py::nms_pose (:241-267): greedy, order-dependent suppression inside one sample -> one thread per sample
// walks the joints exactly like the reference's Python loop (distances on the ORIGINAL coordinates, `nearby` includes the
// joint itself and already-suppressed joints, first maximum wins ties).
__global__ void __launch_bounds__(64) k_nms_pose(const float* __restrict__ preds, const float* __restrict__ maxvals,
                                                 float* __restrict__ out, uint8_t* __restrict__ keep, int B, int K, float thr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = preds + (size_t)b * K * 2;
    const float* v = maxvals + (size_t)b * K;
    uint8_t* kp = keep + (size_t)b * K;
    for (int k = 0; k < K; ++k) kp[k] = 1;
    for (int k = 0; k < K; ++k) {
        if (!kp[k]) continue;
        int count = 0, best = -1;
        float bv = -INFINITY;
        for (int j = 0; j < K; ++j) {
            const float dx = p[2 * j] - p[2 * k], dy = p[2 * j + 1] - p[2 * k + 1];
            if (sqrtf(dx * dx + dy * dy) < thr) {
                ++count;
                if (v[j] > bv) { bv = v[j]; best = j; }
            }
        }
        if (count > 1)
            for (int j = 0; j < K; ++j) {
                const float dx = p[2 * j] - p[2 * k], dy = p[2 * j + 1] - p[2 * k + 1];
                if (sqrtf(dx * dx + dy * dy) < thr && j != best) kp[j] = 0;
            }
    }
    for (int k = 0; k < K; ++k) {
        const float m = kp[k] ? 1.f : 0.f;
        out[((size_t)b * K + k) * 2] = p[2 * k] * m;
        out[((size_t)b * K + k) * 2 + 1] = p[2 * k + 1] * m;
    }
}
extern "C" int pk_nms_pose(const float* preds, const float* maxvals, float* out, uint8_t* keep, int B, int K, float distance_threshold,
                           void* stream) {
    PK_REQUIRE(preds && maxvals && out && keep && B > 0 && K > 0, "pk_nms_pose: bad argument");
    hipLaunchKernelGGL(k_nms_pose, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, preds, maxvals, out, keep, B, K, distance_threshold);
    return pk_launch_status("pk_nms_pose");
}
