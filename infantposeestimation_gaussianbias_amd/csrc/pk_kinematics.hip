// Limb kinematics of pose sequences (this project's own specification: DESIGN.md "Limb kinematics").  The reference prints an asymmetry ratio
// of two amplitudes (examples/quick_start.py:242-249) and stops; a quantitative general-movement assessment also asks for joint angles, for
// how the left and the right limb move together, and for how complex a movement is.  Five entries and one size query:
//   pk_joint_angles     one thread per (sequence, frame, angle): the unsigned interior angle at the middle joint of a triple
//   pk_joint_speeds     one thread per (sequence, frame, joint): the length of the step to the next frame
//   pk_series_stats     one workgroup per (sequence, series), two passes: n, min, max, mean, sd, path, steps, largest step
//   pk_series_xcorr     one workgroup per (sequence, pair, lag): Pearson's r of the co-valid pairs of that lag; then one workgroup per
//                       (sequence, pair) for the summary of the stored r
//   pk_sample_entropy   one workgroup per (sequence, series, tile): a KIN_TILE x KIN_TILE block of template pairs; then one workgroup per
//                       (sequence, series) adds the tiles' integer counts
// A series is a float64 array (S,T,Q); an element is valid iff it is finite (the first two entries write NaN for "no value").
// No float atomics, no global atomics.  Every floating-point sum is taken in the fixed order of the analysis units: thread i of 256 takes
// elements i, i + 256, ... in ascending order, then `block_reduce` (pk_common.h), so two launches give identical bits.  Everything is float64
// on exactly widened inputs, one rounding per operation (-ffp-contract=off: no FMA).
#include "pk_common.h"

#define KIN_THREADS 256
#define KIN_WAVES (KIN_THREADS / PK_WAVE)
#define KIN_TILE PK_KIN_ENTROPY_TILE         // template starts of one side of an entropy tile: one per thread
static_assert(KIN_TILE == KIN_THREADS, "k_sampen_tile gives every thread one template start of the tile's i side");

// ================================================================================================ joint angles and speeds
// Thread idx = (s T + t) A + j.  A triple outside [0, K), or with a == b or b == c, gives NaN without a read (the op layer refuses it).
// u = p_a - p_b, v = p_c - p_b, cr = u.x v.y - u.y v.x, dt = u.x v.x + u.y v.y, theta = atan2(|cr|, dt) in [0, pi].  NaN when one of the three
// joints is invalid by `seq_frame`'s rule or a ray has no length.
__global__ void __launch_bounds__(KIN_THREADS) k_joint_angles(const float* __restrict__ coords, const float* __restrict__ conf,
                                                              const int32_t* __restrict__ triples, double* __restrict__ angles, int64_t total,
                                                              int K, int A, float min_conf) {
    const int64_t idx = (int64_t)blockIdx.x * KIN_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int64_t st = idx / A;
    const int j = (int)(idx - st * A);
    const int a = triples[3 * j], b = triples[3 * j + 1], c = triples[3 * j + 2];
    double theta = NAN;
    if (a >= 0 && a < K && b >= 0 && b < K && c >= 0 && c < K && a != b && b != c) {
        const size_t base = (size_t)st * K;
        const SeqFrame pa = seq_frame(coords, conf, base + a, K, 0, min_conf), pb = seq_frame(coords, conf, base + b, K, 0, min_conf),
                       pc = seq_frame(coords, conf, base + c, K, 0, min_conf);
        if (pa.ok && pb.ok && pc.ok) {
            const double ux = pa.x - pb.x, uy = pa.y - pb.y, vx = pc.x - pb.x, vy = pc.y - pb.y;
            const double cr = ux * vy - uy * vx, dt = ux * vx + uy * vy;
            if (ux * ux + uy * uy > 0.0 && vx * vx + vy * vy > 0.0) theta = atan2(fabs(cr), dt);
        }
    }
    angles[idx] = theta;
}

// Thread idx = (s T + t) K + k: sqrt(dx dx + dy dy) of p[t+1] - p[t] when both frames are valid, else NaN (the last frame always).
__global__ void __launch_bounds__(KIN_THREADS) k_joint_speeds(const float* __restrict__ coords, const float* __restrict__ conf,
                                                              double* __restrict__ speeds, int64_t total, int T, int K, float min_conf) {
    const int64_t idx = (int64_t)blockIdx.x * KIN_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int t = (int)((idx / K) % T);
    double v = NAN;
    if (t + 1 < T) {
        const SeqFrame p = seq_frame(coords, conf, (size_t)idx, K, 0, min_conf), n = seq_frame(coords, conf, (size_t)idx, K, 1, min_conf);
        if (p.ok && n.ok) {
            const double dx = n.x - p.x, dy = n.y - p.y;
            v = sqrt(dx * dx + dy * dy);
        }
    }
    speeds[idx] = v;
}

static int kin_point_grid(const char* who, int64_t total, unsigned* blocks) {
    const int64_t nb = (total + KIN_THREADS - 1) / KIN_THREADS;
    PK_SUPPORTED(nb <= 0x7fffffff, "%s: %lld outputs exceed one launch; take the sequences in parts", who, (long long)total);
    *blocks = (unsigned)nb;
    return PK_OK;
}

extern "C" int pk_joint_angles(const float* coords, const float* conf, const int32_t* triples, double* angles, int S, int T, int K, int A,
                               float min_conf, void* stream) {
    PK_REQUIRE(coords && triples && angles, "pk_joint_angles: null pointer");
    if (const int rc = seq_shape_check("pk_joint_angles", S, T, K)) return rc;
    PK_REQUIRE(A >= 1 && A <= PK_KIN_MAX_ANGLES, "pk_joint_angles: %d angles (1 to %d)", A, PK_KIN_MAX_ANGLES);
    const int64_t total = (int64_t)S * T * A;
    unsigned blocks;
    if (const int rc = kin_point_grid("pk_joint_angles", total, &blocks)) return rc;
    hipLaunchKernelGGL(k_joint_angles, dim3(blocks), dim3(KIN_THREADS), 0, (hipStream_t)stream, coords, conf, triples, angles, total, K, A, min_conf);
    return pk_launch_status("pk_joint_angles");
}

extern "C" int pk_joint_speeds(const float* coords, const float* conf, double* speeds, int S, int T, int K, float min_conf, void* stream) {
    PK_REQUIRE(coords && speeds, "pk_joint_speeds: null pointer");
    if (const int rc = seq_shape_check("pk_joint_speeds", S, T, K)) return rc;
    const int64_t total = (int64_t)S * T * K;
    unsigned blocks;
    if (const int rc = kin_point_grid("pk_joint_speeds", total, &blocks)) return rc;
    hipLaunchKernelGGL(k_joint_speeds, dim3(blocks), dim3(KIN_THREADS), 0, (hipStream_t)stream, coords, conf, speeds, total, T, K, min_conf);
    return pk_launch_status("pk_joint_speeds");
}

// ================================================================================================ statistics of a series
// Element t of the series at `x` (its first element; consecutive elements lie Q apart)
__device__ __forceinline__ double series_at(const double* __restrict__ x, int Q, int t) { return x[(size_t)t * Q]; }

// Pass 1: n, min, max, sum x, and over the steps t -> t+1 with both ends valid sum |x[t+1] - x[t]|, their number and the largest; the
// thread that owns t takes the step that starts at t.  mean = sum / n is stored, and pass 2 subtracts that stored value:
// sd = sqrt(sum (x - mean)^2 / n).
__global__ void __launch_bounds__(KIN_THREADS) k_series_stats(const double* __restrict__ series, double* __restrict__ stats, int T, int Q) {
    __shared__ double red_d[KIN_WAVES];
    __shared__ int red_i[KIN_WAVES];
    const int s = blockIdx.x / Q, q = blockIdx.x - s * Q;
    const double* __restrict__ x = series + (size_t)s * T * Q + q;
    int n_valid = 0, n_steps = 0;
    double lo = INFINITY, hi = -INFINITY, sum = 0.0, path = 0.0, max_step = 0.0;
    for (int t = threadIdx.x; t < T; t += KIN_THREADS) {
        const double v = series_at(x, Q, t);
        if (!isfinite(v)) continue;
        ++n_valid;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        sum += v;
        if (t + 1 >= T) continue;
        const double w = series_at(x, Q, t + 1);
        if (!isfinite(w)) continue;
        const double step = fabs(w - v);
        ++n_steps;
        path += step;
        max_step = step > max_step ? step : max_step;
    }
    const int n = block_reduce<KIN_WAVES>(n_valid, red_i, SumOp()), ns = block_reduce<KIN_WAVES>(n_steps, red_i, SumOp());
    const double tlo = block_reduce<KIN_WAVES>(lo, red_d, MinOp()), thi = block_reduce<KIN_WAVES>(hi, red_d, MaxOp()),
                 tsum = block_reduce<KIN_WAVES>(sum, red_d, SumOp()), tpath = block_reduce<KIN_WAVES>(path, red_d, SumOp()),
                 tmax = block_reduce<KIN_WAVES>(max_step, red_d, MaxOp());
    const double mean = n ? tsum / (double)n : 0.0;
    double ss = 0.0;
    for (int t = threadIdx.x; t < T; t += KIN_THREADS) {
        const double v = series_at(x, Q, t);
        if (!isfinite(v)) continue;
        const double d = v - mean;
        ss += d * d;
    }
    const double tss = block_reduce<KIN_WAVES>(ss, red_d, SumOp());
    if (threadIdx.x == 0) {
        double* o = stats + (size_t)blockIdx.x * PK_KIN_STATS_COLS;
        o[0] = (double)n;
        o[1] = n ? tlo : 0.0;
        o[2] = n ? thi : 0.0;
        o[3] = mean;
        o[4] = n ? sqrt(tss / (double)n) : 0.0;
        o[5] = tpath;
        o[6] = (double)ns;
        o[7] = tmax;
    }
}

extern "C" int pk_series_stats(const double* series, double* stats, int S, int T, int Q, void* stream) {
    PK_REQUIRE(series && stats, "pk_series_stats: null pointer");
    if (const int rc = seq_shape_check("pk_series_stats", S, T, Q)) return rc;
    hipLaunchKernelGGL(k_series_stats, dim3(S * Q), dim3(KIN_THREADS), 0, (hipStream_t)stream, series, stats, T, Q);
    return pk_launch_status("pk_series_stats");
}

// ================================================================================================ cross-correlation over lags
// Workgroup (s, p, l'), lag l = l' - L.  The pairs of a lag are walked by u = the EARLIER of their two frames, 0 <= u < T - |l|:
//   l >= 0: x = x_i[u], y = x_j[u + l];   l < 0: x = x_i[u - l], y = x_j[u]
// so that (i, j) at l and (j, i) at -l see the same pairs under the same u and give the same bits (a product and sxx syy commute).  Thread
// i takes u = i, i + 256, ...: the order of every sum depends on T and l alone, never on S, P, L or the other lags.  Pass 1: n, sum x,
// sum y; mx, my; pass 2: sxx, syy, sxy about those means; r = sxy / sqrt(sxx syy), 0 when n < 2 or not sxx syy > 0.  A pair outside
// [0, Q) (refused by the op layer) gets r = 0 and count 0 without a read.
__global__ void __launch_bounds__(KIN_THREADS) k_series_xcorr(const double* __restrict__ series, const int32_t* __restrict__ pairs,
                                                              double* __restrict__ corr, int32_t* __restrict__ count, int T, int Q, int P,
                                                              int L) {
    __shared__ double red_d[KIN_WAVES];
    __shared__ int red_i[KIN_WAVES];
    const int NL = 2 * L + 1;
    const unsigned sp = blockIdx.x / (unsigned)NL;
    const int li = (int)(blockIdx.x - sp * (unsigned)NL), lag = li - L, s = (int)(sp / (unsigned)P), p = (int)(sp - (unsigned)s * P);
    const int qi = pairs[2 * p], qj = pairs[2 * p + 1];
    const int span = T - (lag < 0 ? -lag : lag);                  // pairs of this lag, valid or not; <= 0: none
    if (qi < 0 || qi >= Q || qj < 0 || qj >= Q || span <= 0) {    // uniform over the block
        if (threadIdx.x == 0) corr[blockIdx.x] = 0.0, count[blockIdx.x] = 0;
        return;
    }
    const double* __restrict__ xi = series + (size_t)s * T * Q + qi + (size_t)(lag < 0 ? -lag : 0) * Q;
    const double* __restrict__ xj = series + (size_t)s * T * Q + qj + (size_t)(lag > 0 ? lag : 0) * Q;
    int n_pairs = 0;
    double sx = 0.0, sy = 0.0;
    for (int u = threadIdx.x; u < span; u += KIN_THREADS) {
        const double x = series_at(xi, Q, u), y = series_at(xj, Q, u);
        if (!(isfinite(x) && isfinite(y))) continue;
        ++n_pairs;
        sx += x;
        sy += y;
    }
    const int n = block_reduce<KIN_WAVES>(n_pairs, red_i, SumOp());
    const double tx = block_reduce<KIN_WAVES>(sx, red_d, SumOp()), ty = block_reduce<KIN_WAVES>(sy, red_d, SumOp());
    if (n < 2) {                                                  // uniform over the block
        if (threadIdx.x == 0) corr[blockIdx.x] = 0.0, count[blockIdx.x] = n;
        return;
    }
    const double mx = tx / (double)n, my = ty / (double)n;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int u = threadIdx.x; u < span; u += KIN_THREADS) {
        const double x = series_at(xi, Q, u), y = series_at(xj, Q, u);
        if (!(isfinite(x) && isfinite(y))) continue;
        const double dx = x - mx, dy = y - my;
        sxx += dx * dx;
        syy += dy * dy;
        sxy += dx * dy;
    }
    const double txx = block_reduce<KIN_WAVES>(sxx, red_d, SumOp()), tyy = block_reduce<KIN_WAVES>(syy, red_d, SumOp()),
                 txy = block_reduce<KIN_WAVES>(sxy, red_d, SumOp());
    if (threadIdx.x == 0) {
        const double den = txx * tyy;
        corr[blockIdx.x] = den > 0.0 ? txy / sqrt(den) : 0.0;
        count[blockIdx.x] = n;
    }
}

// One workgroup per (s, p), from the STORED r and counts, over the lags with count >= min_count: r at lag 0 (0 when that lag does not
// qualify), the lag of the largest r (the lowest l' among equal maxima), that r and that lag's count; 0, 0, 0 without a qualifying lag.
// Exact in any order.
__global__ void __launch_bounds__(KIN_THREADS) k_xcorr_summary(const double* __restrict__ corr, const int32_t* __restrict__ count,
                                                               double* __restrict__ summary, int L, int min_count) {
    __shared__ double best_r[KIN_WAVES];
    __shared__ int best_l[KIN_WAVES];
    const int NL = 2 * L + 1;
    const double* __restrict__ r = corr + (size_t)blockIdx.x * NL;
    const int32_t* __restrict__ c = count + (size_t)blockIdx.x * NL;
    double br = -INFINITY;
    int bl = 0x7fffffff;
    for (int l = threadIdx.x; l < NL; l += KIN_THREADS)
        if (c[l] >= min_count && r[l] > br) br = r[l], bl = l;   // ascending l: the first of equal maxima stays
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double orr = __shfl_xor(br, o, 64);
        const int ol = __shfl_xor(bl, o, 64);
        if (orr > br || (orr == br && ol < bl)) br = orr, bl = ol;
    }
    if ((threadIdx.x & 63) == 0) best_r[threadIdx.x >> 6] = br, best_l[threadIdx.x >> 6] = bl;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < KIN_WAVES; ++w)
            if (best_r[w] > br || (best_r[w] == br && best_l[w] < bl)) br = best_r[w], bl = best_l[w];
        double* o = summary + (size_t)blockIdx.x * 4;
        const bool some = bl < NL;
        o[0] = c[L] >= min_count ? r[L] : 0.0;
        o[1] = some ? (double)(bl - L) : 0.0;
        o[2] = some ? br : 0.0;
        o[3] = some ? (double)c[bl] : 0.0;
    }
}

extern "C" int pk_series_xcorr(const double* series, const int32_t* pairs, double* corr, int32_t* count, double* summary, int S, int T, int Q,
                               int P, int max_lag, int min_count, void* stream) {
    PK_REQUIRE(series && pairs && corr && count && summary, "pk_series_xcorr: null pointer");
    if (const int rc = seq_shape_check("pk_series_xcorr", S, T, Q)) return rc;
    PK_REQUIRE(P >= 1, "pk_series_xcorr: %d pairs (at least 1)", P);
    PK_REQUIRE(max_lag >= 0 && max_lag <= PK_KIN_MAX_LAG, "pk_series_xcorr: max_lag %d (0 to %d)", max_lag, PK_KIN_MAX_LAG);
    PK_REQUIRE(min_count >= 2, "pk_series_xcorr: min_count %d (at least 2: one pair has no correlation)", min_count);
    const int64_t groups = (int64_t)S * P * (2 * max_lag + 1);
    PK_SUPPORTED(groups <= 0x7fffffff, "pk_series_xcorr: %lld (sequence, pair, lag) workgroups exceed one launch; take the pairs in parts",
                 (long long)groups);
    hipLaunchKernelGGL(k_series_xcorr, dim3((unsigned)groups), dim3(KIN_THREADS), 0, (hipStream_t)stream, series, pairs, corr, count, T, Q, P,
                       max_lag);
    const int rc = pk_launch_status("pk_series_xcorr");
    if (rc != PK_OK) return rc;
    hipLaunchKernelGGL(k_xcorr_summary, dim3(S * P), dim3(KIN_THREADS), 0, (hipStream_t)stream, corr, count, summary, max_lag, min_count);
    return pk_launch_status("pk_series_xcorr");
}

// ================================================================================================ sample entropy
// Template start i (0 <= i <= T - m - 1) is in W iff x[i .. i + m] are all valid.  The starts are cut into blocks of KIN_TILE; tile
// (ib, jb), ib <= jb, holds the pairs i in block ib, j in block jb, i < j.  Row ib of the triangle has nb - ib tiles, so tile number
// first(ib) + (jb - ib) with first(ib) = ib nb - ib (ib - 1) / 2, and there are nb (nb + 1) / 2 of them.
static inline int sampen_blocks(int T, int m) { return T - m <= 0 ? 0 : (T - m + KIN_TILE - 1) / KIN_TILE; }

extern "C" int pk_sample_entropy_tiles(int T, int m) {
    if (T <= 0 || T > PK_KIN_MAX_T || m < 1 || m > PK_KIN_MAX_M) return 0;
    const int nb = sampen_blocks(T, m);                           // <= 1024: the product fits
    return nb * (nb + 1) / 2;
}

// One workgroup per (s, q, tile), the tile number in grid x (it passes 65 535 from T - m = 92 417 on, which grid y and z cannot hold).
// Thread i keeps ITS template x[i .. i + m] of block ib in registers; block jb's KIN_TILE + m elements go through LDS with the validity of
// each start; then all threads walk the 256 starts j of the tile together: every lane reads the same LDS address (a broadcast, no bank
// conflict) and compares its own template with it.  B counts max_{k<m} |x[i+k] - x[j+k]| <= tol, A the same over k <= m; the maximum is
// at most tol iff every term is, and fabs(a - b) <= tol is false for a NaN, so an invalid i is one NaN in its registers.  Counts per
// thread <= 256, per workgroup <= 65 536: int32, widened where they are stored.  Integer sums: exact in any order.
template <int M>
__global__ void __launch_bounds__(KIN_THREADS) k_sampen_tile(const double* __restrict__ series, const double* __restrict__ tol,
                                                             int64_t* __restrict__ workspace, int T, int Q, int nb, int tiles) {
    __shared__ double xs[KIN_TILE + PK_KIN_MAX_M];
    __shared__ int okj[KIN_TILE];
    __shared__ int red_i[KIN_WAVES];
    const unsigned sq = blockIdx.x / (unsigned)tiles;
    const int tile = (int)(blockIdx.x - sq * (unsigned)tiles), s = (int)(sq / (unsigned)Q), q = (int)(sq - (unsigned)s * Q), tid = threadIdx.x;
    int64_t* __restrict__ row = workspace + (size_t)blockIdx.x * 2;
    const double tl = tol[sq];
    if (!(isfinite(tl) && tl >= 0.0)) {                           // uniform over the block
        if (tid == 0) row[0] = 0, row[1] = 0;
        return;
    }
    // (ib, jb) of the tile: the root of first(ib) = tile as a guess, corrected in integers
    const double e = 2.0 * nb + 1.0;
    int ib = (int)((e - sqrt(e * e - 8.0 * (double)tile)) * 0.5);
    ib = ib < 0 ? 0 : (ib > nb - 1 ? nb - 1 : ib);
    while (ib > 0 && ib * nb - ib * (ib - 1) / 2 > tile) --ib;
    while (ib + 1 < nb && (ib + 1) * nb - (ib + 1) * ib / 2 <= tile) ++ib;
    const int jb = ib + (tile - (ib * nb - ib * (ib - 1) / 2));

    const double* __restrict__ x = series + (size_t)s * T * Q + q;
    const int i0 = ib * KIN_TILE + tid, j0 = jb * KIN_TILE;       // < 2^18 + 2^8
    double xi[M + 1];
    bool oki = true;
#pragma unroll
    for (int k = 0; k <= M; ++k) {
        xi[k] = i0 + k < T ? series_at(x, Q, i0 + k) : NAN;
        oki = oki && isfinite(xi[k]);
    }
    if (!oki) xi[0] = NAN;                                        // m >= 1: term 0 is in both counts
    xs[tid] = j0 + tid < T ? series_at(x, Q, j0 + tid) : NAN;
    if (tid < M) xs[KIN_TILE + tid] = j0 + KIN_TILE + tid < T ? series_at(x, Q, j0 + KIN_TILE + tid) : NAN;
    __syncthreads();
    {
        bool ok = true;                                           // a start beyond T - m - 1 reaches an element beyond T: NaN
#pragma unroll
        for (int k = 0; k <= M; ++k) ok = ok && isfinite(xs[tid + k]);
        okj[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    const int after = ib == jb ? tid : -1;                        // the diagonal tile keeps j > i
    int cb = 0, ca = 0;
#pragma unroll 8
    for (int jj = 0; jj < KIN_TILE; ++jj) {
        bool b = okj[jj] != 0 && jj > after;
#pragma unroll
        for (int k = 0; k < M; ++k) b = b && fabs(xi[k] - xs[jj + k]) <= tl;
        const bool a = b && fabs(xi[M] - xs[jj + M]) <= tl;
        cb += b ? 1 : 0;
        ca += a ? 1 : 0;
    }
    const int tb = block_reduce<KIN_WAVES>(cb, red_i, SumOp()), ta = block_reduce<KIN_WAVES>(ca, red_i, SumOp());
    if (tid == 0) row[0] = tb, row[1] = ta;
}

// One workgroup per (s, q): |W| from the series, B and A as the sum of the tiles' rows; (|W|, 0, 0) for a tolerance that is not finite or
// is negative.
__global__ void __launch_bounds__(KIN_THREADS) k_sampen_reduce(const double* __restrict__ series, const double* __restrict__ tol,
                                                               const int64_t* __restrict__ workspace, int64_t* __restrict__ counts, int T,
                                                               int Q, int m, int tiles) {
    __shared__ long long red_l[KIN_WAVES];
    const int s = blockIdx.x / Q, q = blockIdx.x - s * Q;
    const double* __restrict__ x = series + (size_t)s * T * Q + q;
    long long nw = 0, cb = 0, ca = 0;
    for (int i = threadIdx.x; i < T - m; i += KIN_THREADS) {
        bool ok = true;
        for (int k = 0; k <= m; ++k) ok = ok && isfinite(series_at(x, Q, i + k));
        nw += ok ? 1 : 0;
    }
    const int64_t* __restrict__ rows = workspace + (size_t)blockIdx.x * tiles * 2;
    for (int t = threadIdx.x; t < tiles; t += KIN_THREADS) {
        cb += rows[2 * (size_t)t];
        ca += rows[2 * (size_t)t + 1];
    }
    const long long tw = block_reduce<KIN_WAVES>(nw, red_l, SumOp()), tb = block_reduce<KIN_WAVES>(cb, red_l, SumOp()),
                    ta = block_reduce<KIN_WAVES>(ca, red_l, SumOp());
    if (threadIdx.x == 0) {
        const double tl = tol[blockIdx.x];
        const bool live = isfinite(tl) && tl >= 0.0;
        int64_t* o = counts + (size_t)blockIdx.x * 3;
        o[0] = tw;
        o[1] = live ? tb : 0;
        o[2] = live ? ta : 0;
    }
}

extern "C" int pk_sample_entropy(const double* series, const double* tol, int64_t* workspace, int64_t* counts, int S, int T, int Q, int m,
                                 void* stream) {
    PK_REQUIRE(series && tol && workspace && counts, "pk_sample_entropy: null pointer");
    if (const int rc = seq_shape_check("pk_sample_entropy", S, T, Q)) return rc;
    PK_REQUIRE(m >= 1 && m <= PK_KIN_MAX_M, "pk_sample_entropy: template length m=%d (1 to %d)", m, PK_KIN_MAX_M);
    PK_SUPPORTED(T <= PK_KIN_MAX_T, "pk_sample_entropy: T=%d frames exceed the %d of one call (the pair count is quadratic); analyse it in windows", T,
                 PK_KIN_MAX_T);
    const int nb = sampen_blocks(T, m), tiles = pk_sample_entropy_tiles(T, m);
    const int64_t groups = (int64_t)S * Q * tiles;
    PK_SUPPORTED(groups <= 0x7fffffff, "pk_sample_entropy: %lld (sequence, series, tile) workgroups exceed one launch; take the series in parts",
                 (long long)groups);
    if (tiles > 0) {
        const dim3 grid((unsigned)groups), block(KIN_THREADS);
        switch (m) {
            case 1: hipLaunchKernelGGL(k_sampen_tile<1>, grid, block, 0, (hipStream_t)stream, series, tol, workspace, T, Q, nb, tiles); break;
            case 2: hipLaunchKernelGGL(k_sampen_tile<2>, grid, block, 0, (hipStream_t)stream, series, tol, workspace, T, Q, nb, tiles); break;
            case 3: hipLaunchKernelGGL(k_sampen_tile<3>, grid, block, 0, (hipStream_t)stream, series, tol, workspace, T, Q, nb, tiles); break;
            default: hipLaunchKernelGGL(k_sampen_tile<4>, grid, block, 0, (hipStream_t)stream, series, tol, workspace, T, Q, nb, tiles); break;
        }
        const int rc = pk_launch_status("pk_sample_entropy");
        if (rc != PK_OK) return rc;
    }
    hipLaunchKernelGGL(k_sampen_reduce, dim3(S * Q), dim3(KIN_THREADS), 0, (hipStream_t)stream, series, tol, workspace, counts, T, Q, m, tiles);
    return pk_launch_status("pk_sample_entropy");
}
