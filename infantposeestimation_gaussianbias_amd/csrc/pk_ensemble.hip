// Stochastic-depth ensembles (this project's own specification: DESIGN.md "Predictive uncertainty").  The reference's
// UncertaintyAnalyzer.monte_carlo_dropout_uncertainty (analysis/advanced_analysis.py:430-485) runs 30 batch-1 forwards, copies each to the
// host and takes np.mean / np.std there.  Here the S members are one stack on the device and two kernels read it:
//   pk_ensemble_moments   per-element mean and standard deviation over the members: a streaming kernel, S L floats in, 2 L out
//   pk_ensemble_points    per point: mean, covariance and its 1-sigma ellipse, confidence statistics and agreement over the members
// No atomics; every floating-point sum is taken in a fixed order (the arithmetic is written out in include/posekernels.h): same bits each run.
#include "pk_rowops.h"

#define ENS_THREADS 256                                           // the analysis units' workgroup
#define ENS_WAVES (ENS_THREADS / PK_WAVE)

// ================================================================================================ moments over the members
// V floats per thread and pass: 4 (one 16-byte load per member) or 1.
template <int V> struct EnsGroup;
template <> struct EnsGroup<4> {
    f32x4 v;
    __device__ __forceinline__ float at(int j) const { return v[j]; }
    __device__ __forceinline__ void set(int j, float x) { v[j] = x; }
};
template <> struct EnsGroup<1> {
    float v;
    __device__ __forceinline__ float at(int) const { return v; }
    __device__ __forceinline__ void set(int, float x) { v = x; }
};

// S <= PK_ENS_REG_MEMBERS: every member of the group is loaded once and stays in registers for both sums (the loop bounds are constants,
// so the array never leaves the register file; `s < S` is uniform).  stride_g, G: member stride and length in groups of V floats.
template <int V>
__global__ void __launch_bounds__(ENS_THREADS) k_ens_moments_reg(const float* __restrict__ stack, int64_t stride_g, int S, int64_t G,
                                                                 double count, double dof, float* __restrict__ mean,
                                                                 float* __restrict__ sdev) {
    typedef EnsGroup<V> Grp;
    const Grp* __restrict__ src = (const Grp*)stack;
    for (int64_t g = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x; g < G; g += (int64_t)gridDim.x * ENS_THREADS) {
        Grp m[PK_ENS_REG_MEMBERS];
#pragma unroll
        for (int s = 0; s < PK_ENS_REG_MEMBERS; ++s)
            if (s < S) m[s] = src[(int64_t)s * stride_g + g];
        Grp om, os;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            double sum = 0.0;
#pragma unroll
            for (int s = 0; s < PK_ENS_REG_MEMBERS; ++s)
                if (s < S) sum += (double)m[s].at(j);
            const double mu = sum / count;
            double q = 0.0;
#pragma unroll
            for (int s = 0; s < PK_ENS_REG_MEMBERS; ++s)
                if (s < S) {
                    const double d = (double)m[s].at(j) - mu;
                    q += d * d;
                }
            om.set(j, (float)mu);
            os.set(j, (float)sqrt(q / dof));
        }
        ((Grp*)mean)[g] = om;
        ((Grp*)sdev)[g] = os;
    }
}

// Any S: the sum, then the squares in a second read of the same lines (a thread re-reads exactly what it read, S 16-byte words, which
// L2 still holds).  Four members' loads are issued together.
template <int V>
__global__ void __launch_bounds__(ENS_THREADS) k_ens_moments_two(const float* __restrict__ stack, int64_t stride_g, int S, int64_t G,
                                                                 double count, double dof, float* __restrict__ mean,
                                                                 float* __restrict__ sdev) {
    typedef EnsGroup<V> Grp;
    const Grp* __restrict__ src = (const Grp*)stack;
    for (int64_t g = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x; g < G; g += (int64_t)gridDim.x * ENS_THREADS) {
        double sum[V], q[V], mu[V];
#pragma unroll
        for (int j = 0; j < V; ++j) sum[j] = 0.0, q[j] = 0.0;
        int s = 0;
        for (; s + 4 <= S; s += 4) {
            Grp a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = src[(int64_t)(s + u) * stride_g + g];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < V; ++j) sum[j] += (double)a[u].at(j);
        }
        for (; s < S; ++s) {
            const Grp a = src[(int64_t)s * stride_g + g];
#pragma unroll
            for (int j = 0; j < V; ++j) sum[j] += (double)a.at(j);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) mu[j] = sum[j] / count;
        for (s = 0; s + 4 <= S; s += 4) {
            Grp a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = src[(int64_t)(s + u) * stride_g + g];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const double d = (double)a[u].at(j) - mu[j];
                    q[j] += d * d;
                }
        }
        for (; s < S; ++s) {
            const Grp a = src[(int64_t)s * stride_g + g];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double d = (double)a.at(j) - mu[j];
                q[j] += d * d;
            }
        }
        Grp om, os;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            om.set(j, (float)mu[j]);
            os.set(j, (float)sqrt(q[j] / dof));
        }
        ((Grp*)mean)[g] = om;
        ((Grp*)sdev)[g] = os;
    }
}

static inline bool ens_apart(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a1 <= b0 || b1 <= a0; }

extern "C" int pk_ensemble_moments(const float* stack, int64_t member_stride, int S, int64_t L, int ddof, float* mean, float* std,
                                   void* stream) {
    PK_REQUIRE(stack && mean && std, "pk_ensemble_moments: null pointer");
    PK_REQUIRE(ddof == 0 || ddof == 1, "pk_ensemble_moments: ddof %d (0 or 1)", ddof);
    PK_REQUIRE(S >= 1 + ddof, "pk_ensemble_moments: %d members with ddof=%d (at least %d)", S, ddof, 1 + ddof);
    PK_REQUIRE(L >= 1, "pk_ensemble_moments: bad length L=%lld", (long long)L);
    PK_REQUIRE(member_stride >= L, "pk_ensemble_moments: member_stride=%lld below L=%lld", (long long)member_stride, (long long)L);
    PK_REQUIRE(L <= (int64_t)1 << 40 && member_stride <= ((int64_t)1 << 60) / S, "pk_ensemble_moments: stack too large S=%d member_stride=%lld L=%lld",
               S, (long long)member_stride, (long long)L);
    const uintptr_t s0 = (uintptr_t)stack, s1 = s0 + ((size_t)(S - 1) * member_stride + L) * 4;
    const uintptr_t m0 = (uintptr_t)mean, m1 = m0 + (size_t)L * 4, d0 = (uintptr_t)std, d1 = d0 + (size_t)L * 4;
    PK_REQUIRE(ens_apart(s0, s1, m0, m1) && ens_apart(s0, s1, d0, d1), "pk_ensemble_moments: an output overlaps the stack");
    PK_REQUIRE(ens_apart(m0, m1, d0, d1), "pk_ensemble_moments: mean and std overlap");
    const bool vec = L % 4 == 0 && member_stride % 4 == 0 && ((s0 | m0 | d0) & 15) == 0;
    const int64_t G = vec ? L / 4 : L, stride_g = vec ? member_stride / 4 : member_stride;
    const int gb = capped_grid((G + ENS_THREADS - 1) / ENS_THREADS, PK_ENS_GRID_CAP);
    const double count = (double)S, dof = (double)(S - ddof);
    const bool reg = S <= PK_ENS_REG_MEMBERS;
#define ENS_LAUNCH(kernel) \
    hipLaunchKernelGGL(kernel, dim3(gb), dim3(ENS_THREADS), 0, (hipStream_t)stream, stack, stride_g, S, G, count, dof, mean, std)
    if (vec && reg) ENS_LAUNCH(k_ens_moments_reg<4>);
    else if (vec) ENS_LAUNCH(k_ens_moments_two<4>);
    else if (reg) ENS_LAUNCH(k_ens_moments_reg<1>);
    else ENS_LAUNCH(k_ens_moments_two<1>);
#undef ENS_LAUNCH
    return pk_launch_status("pk_ensemble_moments");
}

// ================================================================================================ one row per point
struct EnsMember { double x, y, c; bool ok; };
__device__ __forceinline__ EnsMember ens_member(const float* __restrict__ coords, const float* __restrict__ conf, int64_t M, int64_t m, int s,
                                                float min_conf) {
    const size_t i = (size_t)s * M + m;
    const float x = coords[2 * i], y = coords[2 * i + 1];
    EnsMember e;
    e.ok = isfinite(x) && isfinite(y);
    e.c = 0.0;
    if (conf != nullptr) {
        const float c = conf[i];
        e.ok = e.ok && isfinite(c) && c >= min_conf;
        e.c = (double)c;
    }
    e.x = (double)x, e.y = (double)y;
    return e;
}

__global__ void __launch_bounds__(ENS_THREADS) k_ens_points(const float* __restrict__ coords, const float* __restrict__ conf,
                                                            const double* __restrict__ centre, double* __restrict__ out, int S, int64_t M,
                                                            float min_conf, double radius, int ddof) {
    __shared__ double red[ENS_WAVES];
    const double r2 = radius * radius;
    for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {         // uniform over the block
        double n = 0.0, sx = 0.0, sy = 0.0, sc = 0.0, cmin = INFINITY;
        for (int s = threadIdx.x; s < S; s += ENS_THREADS) {
            const EnsMember e = ens_member(coords, conf, M, m, s, min_conf);
            if (e.ok) {
                n += 1.0, sx += e.x, sy += e.y, sc += e.c;
                cmin = e.c < cmin ? e.c : cmin;
            }
        }
        n = block_reduce<ENS_WAVES>(n, red, SumOp());
        sx = block_reduce<ENS_WAVES>(sx, red, SumOp());
        sy = block_reduce<ENS_WAVES>(sy, red, SumOp());
        sc = block_reduce<ENS_WAVES>(sc, red, SumOp());
        cmin = block_reduce<ENS_WAVES>(cmin, red, MinOp());
        double* __restrict__ o = out + (size_t)m * PK_ENS_POINT_COLS;
        if (n < (double)(1 + ddof)) {                             // uniform: every thread holds the same n
            if (threadIdx.x < PK_ENS_POINT_COLS) o[threadIdx.x] = 0.0;
            continue;
        }
        const double mx = sx / n, my = sy / n, mc = sc / n;
        const double cx = centre ? centre[2 * m] : mx, cy = centre ? centre[2 * m + 1] : my;
        double qxx = 0.0, qyy = 0.0, qxy = 0.0, qcc = 0.0, agree = 0.0;
        for (int s = threadIdx.x; s < S; s += ENS_THREADS) {
            const EnsMember e = ens_member(coords, conf, M, m, s, min_conf);
            if (e.ok) {
                const double dx = e.x - mx, dy = e.y - my, dc = e.c - mc, ex = e.x - cx, ey = e.y - cy;
                qxx += dx * dx, qyy += dy * dy, qxy += dx * dy, qcc += dc * dc;
                if (ex * ex + ey * ey <= r2) agree += 1.0;
            }
        }
        qxx = block_reduce<ENS_WAVES>(qxx, red, SumOp());
        qyy = block_reduce<ENS_WAVES>(qyy, red, SumOp());
        qxy = block_reduce<ENS_WAVES>(qxy, red, SumOp());
        qcc = block_reduce<ENS_WAVES>(qcc, red, SumOp());
        agree = block_reduce<ENS_WAVES>(agree, red, SumOp());
        if (threadIdx.x == 0) {
            const double dof = n - (double)ddof;
            const double vx = qxx / dof, vy = qyy / dof, c = qxy / dof;
            const double h = (vx + vy) * 0.5, d = (vx - vy) * 0.5, r = sqrt(d * d + c * c);
            const double lo = h - r;
            o[0] = n, o[1] = mx, o[2] = my, o[3] = vx, o[4] = vy, o[5] = c;
            o[6] = h + r, o[7] = lo > 0.0 ? lo : 0.0;
            o[8] = conf ? mc : 0.0, o[9] = conf ? sqrt(qcc / dof) : 0.0, o[10] = conf ? cmin : 0.0;
            o[11] = agree;
        }
    }
}

extern "C" int pk_ensemble_points(const float* coords, const float* conf, const double* centre, double* out, int S, int64_t M, float min_conf,
                                  double radius, int ddof, void* stream) {
    PK_REQUIRE(coords && out, "pk_ensemble_points: null pointer");
    PK_REQUIRE(S >= 1 && M >= 1 && M < ((int64_t)1 << 61) / S, "pk_ensemble_points: bad shape S=%d M=%lld", S, (long long)M);
    PK_REQUIRE(radius >= 0.0 && radius <= 1.7976931348623157e308, "pk_ensemble_points: radius %g (finite, at least 0)", radius);
    PK_REQUIRE(ddof == 0 || ddof == 1, "pk_ensemble_points: ddof %d (0 or 1)", ddof);
    const int gb = capped_grid(M, PK_ENS_POINT_GRID_CAP);
    hipLaunchKernelGGL(k_ens_points, dim3(gb), dim3(ENS_THREADS), 0, (hipStream_t)stream, coords, conf, centre, out, S, M, min_conf, radius, ddof);
    return pk_launch_status("pk_ensemble_points");
}
