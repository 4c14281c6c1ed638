// Movement frequency spectrum of pose sequences (this project's own specification: DESIGN.md "Movement spectrum").  The reference describes
// its use case by how infants move ("subtle limb movements, low-frequency motions", configs/preemie_optimized.yaml) and builds its clinical
// example from an amplitude and a movement frequency (examples/quick_start.py:221-237), and computes neither; pk_motion_stats gives the
// amplitude, this unit the frequency.  One entry, two launches:
//   k_motion_spectrum    grid (S K, ceil(F / 64)): the windowed, mean-removed Fourier power of one joint at 64 bins of the band
//   k_spectrum_summary   one workgroup per (sequence, joint): band power, peak bin, peak power and centroid from the stored power row
// No float atomics.  Every floating-point sum is taken in a fixed order that depends on T alone (see the kernels), so two launches give
// identical bits and a bin's bits depend neither on S, on K nor on which other bins are in the launch.
#include "pk_common.h"

#define SPEC_THREADS 256
#define SPEC_WAVES (SPEC_THREADS / PK_WAVE)
#define SPEC_BINS PK_WAVE                    // bins of one workgroup: lane l of EVERY wave owns bin blockIdx.y 64 + l
#define SPEC_TILE 256                        // frames of one LDS tile
#define SPEC_CHUNK (SPEC_TILE / SPEC_WAVES)  // wave w takes frames [64 w, 64 w + 64) of every tile
#define SPEC_TWO_PI 6.283185307179586

// Frame t of the joint at `base`, valid by `seq_frame`'s rule (pk_common.h).  `w` is the window weight of a valid frame (0 of an
// invalid one): 1, or the periodic Hann window 0.5 - 0.5 cos(2 pi t / T).
struct SpecFrame { double x, y, w; bool ok; };
__device__ __forceinline__ SpecFrame spec_frame(const float* __restrict__ coords, const float* __restrict__ conf, size_t base, int K, int t, int T,
                                                float min_conf, int window) {
    const SeqFrame p = seq_frame(coords, conf, base, K, t, min_conf);
    SpecFrame f;
    f.ok = p.ok;
    f.x = p.x;
    f.y = p.y;
    f.w = !f.ok ? 0.0 : (window ? 0.5 - 0.5 * cos(SPEC_TWO_PI * ((double)t / (double)T)) : 1.0);
    return f;
}

// Everything float64 on the exactly widened float32 inputs, one rounding per operation (-ffp-contract=off: no FMA).
//   1. n, W = sum w_t, sum w_t x_t, sum w_t y_t over the valid frames: thread i takes frames i, i + 256, ... in ascending order, then
//      `block_reduce` (pk_common.h).  m = (sum w x / W, sum w y / W).  n < 2 or not W > 0: the 64 bins are 0.
//   2. The frames pass through LDS in tiles of 256: thread i stores u_t = w_t (p_t - m) of frame tile + i (0 for an invalid frame, which
//      adds +-0 to every sum).  Wave w then walks frames 64 w .. 64 w + 63 of the tile in ascending order; all its lanes read the same
//      u_t (one address: a broadcast), lane l multiplies it with (cos, sin) of ITS bin's phase and adds to its four sums.  The phase is
//      exact: r = ((j0 + j) t) mod N kept as an integer (advanced by j0 + j <= N / 2 per frame with one conditional subtraction, so it
//      never exceeds 32 bits; its start in a tile by the 64-bit product), ang = 2 pi ((double)r / (double)N) in [0, 2 pi).
//   3. The four waves' sums of a bin are added in wave order, ((s0 + s1) + s2) + s3, and P = (4 / (W W)) ((Xre^2 + Xim^2) + (Yre^2 + Yim^2)).
// So the order of a bin's sum is: frames t with (t mod 256) / 64 == w ascending into wave w's partial sum, then the partial sums in order.
// The workgroups of the first 64 bins also store n and W into columns 0 and 1 of the summary row.
__global__ void __launch_bounds__(SPEC_THREADS) k_motion_spectrum(const float* __restrict__ coords, const float* __restrict__ conf,
                                                                  double* __restrict__ power, double* __restrict__ summary, int T, int K,
                                                                  float min_conf, int N, int j0, int F, int window) {
    __shared__ double red_d[SPEC_WAVES];
    __shared__ int red_i[SPEC_WAVES];
    __shared__ double tile_x[SPEC_TILE], tile_y[SPEC_TILE];
    __shared__ double part[SPEC_WAVES - 1][4][SPEC_BINS];
    const int sk = blockIdx.x, s = sk / K, k = sk - s * K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t base = (size_t)s * T * K + k;                    // frame t of this joint: element base + t K of (S,T,K)
    const int j = blockIdx.y * SPEC_BINS + lane;                  // this lane's bin of the band
    double* __restrict__ prow = power + (size_t)sk * F;

    int n_valid = 0;
    double sw = 0.0, swx = 0.0, swy = 0.0;
    for (int t = threadIdx.x; t < T; t += SPEC_THREADS) {
        const SpecFrame f = spec_frame(coords, conf, base, K, t, T, min_conf, window);
        if (!f.ok) continue;
        ++n_valid;
        sw += f.w;
        swx += f.w * f.x;
        swy += f.w * f.y;
    }
    const int n = block_reduce<SPEC_WAVES>(n_valid, red_i, SumOp());
    const double W = block_reduce<SPEC_WAVES>(sw, red_d, SumOp()), SX = block_reduce<SPEC_WAVES>(swx, red_d, SumOp()),
                 SY = block_reduce<SPEC_WAVES>(swy, red_d, SumOp());
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        summary[(size_t)sk * 6] = (double)n;
        summary[(size_t)sk * 6 + 1] = W;
    }
    if (n < 2 || !(W > 0.0)) {                                    // uniform over the block
        if (wave == 0 && j < F) prow[j] = 0.0;
        return;
    }
    const double mx = SX / W, my = SY / W;

    // jb <= N / 2: lanes past the band repeat its last bin and store nothing
    const unsigned un = (unsigned)N, jb = (unsigned)j0 + (unsigned)(j < F ? j : F - 1);
    const unsigned tile_step = (unsigned)(((uint64_t)jb * SPEC_TILE) % un);   // phase advance of one tile
    unsigned r_tile = (unsigned)(((uint64_t)jb * (unsigned)(wave * SPEC_CHUNK)) % un);      // phase of this wave's first frame of the tile
    double xre = 0.0, xim = 0.0, yre = 0.0, yim = 0.0;
    for (int tile = 0; tile < T; tile += SPEC_TILE) {
        __syncthreads();                                          // the previous tile has been read
        {
            const int t = tile + threadIdx.x;
            double ux = 0.0, uy = 0.0;
            if (t < T) {
                const SpecFrame f = spec_frame(coords, conf, base, K, t, T, min_conf, window);
                if (f.ok) {
                    ux = f.w * (f.x - mx);
                    uy = f.w * (f.y - my);
                }
            }
            tile_x[threadIdx.x] = ux;
            tile_y[threadIdx.x] = uy;
        }
        __syncthreads();
        const int first = wave * SPEC_CHUNK, left = T - tile - first;         // frames of the tile from this wave's first one on
        const int count = left < SPEC_CHUNK ? left : SPEC_CHUNK;              // <= 0: the sequence ended before this wave's chunk
        unsigned r = r_tile;
        for (int i = 0; i < count; ++i) {
            const double ux = tile_x[first + i], uy = tile_y[first + i];
            const double ang = SPEC_TWO_PI * ((double)r / (double)un);
            double sn, cs;
            sincos(ang, &sn, &cs);
            xre += ux * cs;
            xim += ux * sn;
            yre += uy * cs;
            yim += uy * sn;
            r += jb;                                              // < 2^30 + 2^29
            r = r >= un ? r - un : r;
        }
        r_tile += tile_step;
        r_tile = r_tile >= un ? r_tile - un : r_tile;
    }
    if (wave > 0) {
        part[wave - 1][0][lane] = xre;
        part[wave - 1][1][lane] = xim;
        part[wave - 1][2][lane] = yre;
        part[wave - 1][3][lane] = yim;
    }
    __syncthreads();
    if (wave == 0 && j < F) {
#pragma unroll
        for (int w = 0; w < SPEC_WAVES - 1; ++w) {
            xre += part[w][0][lane];
            xim += part[w][1][lane];
            yre += part[w][2][lane];
            yim += part[w][3][lane];
        }
        prow[j] = (4.0 / (W * W)) * ((xre * xre + xim * xim) + (yre * yre + yim * yim));
    }
}

// Columns 2-5 of the summary from the stored power row.  Thread i takes bins i, i + 256, ... in ascending order, then the block
// combines: sums by `block_reduce`, the peak as the largest power with the lowest bin among equal ones (exact in any order).
__global__ void __launch_bounds__(SPEC_THREADS) k_spectrum_summary(const double* __restrict__ power, double* __restrict__ summary, int j0, int F) {
    __shared__ double red_d[SPEC_WAVES];
    __shared__ double best_p[SPEC_WAVES];
    __shared__ int best_j[SPEC_WAVES];
    const double* __restrict__ prow = power + (size_t)blockIdx.x * F;
    double sum = 0.0, moment = 0.0, bp = -1.0;
    int bj = 0x7fffffff;
    for (int j = threadIdx.x; j < F; j += SPEC_THREADS) {
        const double p = prow[j];
        sum += p;
        moment += (double)(j0 + j) * p;
        if (p > bp) bp = p, bj = j;                               // ascending j: the first of equal maxima stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double op = __shfl_xor(bp, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (op > bp || (op == bp && oj < bj)) bp = op, bj = oj;
    }
    if ((threadIdx.x & 63) == 0) best_p[threadIdx.x >> 6] = bp, best_j[threadIdx.x >> 6] = bj;
    // the barriers of block_reduce also publish best_*
    const double total = block_reduce<SPEC_WAVES>(sum, red_d, SumOp()), mom = block_reduce<SPEC_WAVES>(moment, red_d, SumOp());
    if (threadIdx.x == 0) {
        for (int w = 1; w < SPEC_WAVES; ++w)
            if (best_p[w] > bp || (best_p[w] == bp && best_j[w] < bj)) bp = best_p[w], bj = best_j[w];
        double* o = summary + (size_t)blockIdx.x * 6;
        const bool some = total != 0.0 && bj < F;                 // bj stays out of range only if no power compares (NaN)
        o[2] = total;
        o[3] = some ? (double)(j0 + bj) : -1.0;
        o[4] = some ? bp : 0.0;
        o[5] = some ? mom / total : 0.0;
    }
}

extern "C" int pk_motion_spectrum(const float* coords, const float* conf, double* power, double* summary, int S, int T, int K, float min_conf,
                                  int N, int j0, int F, int window, void* stream) {
    PK_REQUIRE(coords && power && summary, "pk_motion_spectrum: null pointer");
    if (const int rc = seq_shape_check("pk_motion_spectrum", S, T, K)) return rc;
    PK_REQUIRE(window == 0 || window == 1, "pk_motion_spectrum: window %d (0 rectangular, 1 Hann)", window);
    PK_REQUIRE(N >= 2 && N <= PK_SPEC_MAX_NFFT, "pk_motion_spectrum: transform length N=%d (2 to %d)", N, PK_SPEC_MAX_NFFT);
    PK_REQUIRE(F >= 1 && F <= PK_SPEC_MAX_BINS, "pk_motion_spectrum: %d bins (1 to %d)", F, PK_SPEC_MAX_BINS);
    PK_REQUIRE(j0 >= 1, "pk_motion_spectrum: first bin j0=%d (the mean is removed: there is no bin 0)", j0);
    PK_REQUIRE((int64_t)j0 + F - 1 <= N / 2, "pk_motion_spectrum: bins %d to %lld lie beyond N / 2 = %d", j0, (long long)j0 + F - 1, N / 2);
    hipLaunchKernelGGL(k_motion_spectrum, dim3(S * K, (F + SPEC_BINS - 1) / SPEC_BINS), dim3(SPEC_THREADS), 0, (hipStream_t)stream, coords, conf,
                       power, summary, T, K, min_conf, N, j0, F, window);
    const int rc = pk_launch_status("pk_motion_spectrum");
    if (rc != PK_OK) return rc;
    hipLaunchKernelGGL(k_spectrum_summary, dim3(S * K), dim3(SPEC_THREADS), 0, (hipStream_t)stream, power, summary, j0, F);
    return pk_launch_status("pk_motion_spectrum");
}
