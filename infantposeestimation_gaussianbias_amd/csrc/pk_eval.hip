// f1: COCO keypoint evaluation (COCOeval with iouType='keypoints', one category, maxDets = [20]) on the device, and the evaluator's
// per-instance records (pk_pose_records, at the end).
//
// The host (utils/coco_eval.py) parses the annotation file, groups ground truths and detections by image (images in ascending id
// order, file / record order inside an image) and computes every CSR offset; the four kernels here do the data-parallel part:
//   k_coco_oks     one workgroup per image: stable score rank of the image's detections (capped at max_dets) + the OKS block (D_i x G_i)
//   k_coco_match   one workgroup per image: one lane per (area range, threshold) runs evaluateImg's sequential greedy scan
//   k_coco_rank    global stable rank of all capped detections by (-score, concatenation position): counting rank over LDS tiles
//   k_coco_accum   one workgroup per (area, threshold) curve: integer prefix sums, fp64 precision / recall, suffix-max envelope and the
//                  searchsorted lookups of the recall thresholds
// No atomics; every floating-point value is computed by one thread in the order numpy computes it (the integer scans are exact and max is
// order-independent), so results are bitwise reproducible.  Floating point follows numpy: -ffp-contract=off (Makefile) and np.sum's
// pairwise order for the OKS sum; only the device exp may differ from glibc's by an ulp.
#include "pk_common.h"

#include <math.h>

#define PK_COCO_MAX_K 64
#define PK_COCO_MAX_DETS 64
#define PK_COCO_MAX_CURVES 64      // A * T lanes of the match kernel (one wave)
#define PK_COCO_GTM_LDS 512        // ground truths per image whose "already matched" flags live in LDS; beyond that: the workspace

// np.sum of n <= 128 float64 terms fed in order: n < 8 left to right; otherwise 8 strided partial sums over the first n - n % 8 terms,
// combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail in order (numpy's pairwise_sum leaf).  The partial sums rotate through
// registers instead of being indexed by the term count.
struct NpSum {
    double r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, r6 = 0, r7 = 0, res = 0;
    int c = 0, m = 0;
    __device__ explicit NpSum(int n) : m(n >= 8 ? n - n % 8 : 0) {}
    __device__ double combine() const { return ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); }
    __device__ void add(double v) {
        if (c < m) {
            const double t = r0 + v;
            r0 = r1; r1 = r2; r2 = r3; r3 = r4; r4 = r5; r5 = r6; r6 = r7; r7 = t;
        } else {
            if (c == m && m > 0) res = combine();
            res += v;
        }
        ++c;
    }
    __device__ double total() const { return (m > 0 && c == m) ? combine() : res; }
};

// ---- OKS: computeOks per image ---------------------------------------------------------------------------------------------------
// gt_kpt (G,K,3), gt_bbox (G,4), gt_area (G); dt_kpt (N,K,3), dt_score (N) grouped by image; vars = (2 sigma)^2 (K).
__global__ void __launch_bounds__(256) k_coco_oks(const double* __restrict__ gt_kpt, const double* __restrict__ gt_bbox,
                                                  const double* __restrict__ gt_area, const int32_t* __restrict__ gt_off,
                                                  const double* __restrict__ dt_kpt, const double* __restrict__ dt_score,
                                                  const int32_t* __restrict__ dt_off, const double* __restrict__ vars,
                                                  const int32_t* __restrict__ cap_off, const int64_t* __restrict__ oks_off,
                                                  int32_t* __restrict__ cap_idx, double* __restrict__ oks, int K, int max_dets) {
    __shared__ int sel[PK_COCO_MAX_DETS];
    __shared__ double svar[PK_COCO_MAX_K];
    const int img = blockIdx.x;
    const int d0 = dt_off[img], n = dt_off[img + 1] - d0;
    const int g0 = gt_off[img], G = gt_off[img + 1] - g0;
    const int D = min(n, max_dets);
    for (int k = threadIdx.x; k < K; k += blockDim.x) svar[k] = vars[k];
    // stable rank of each detection inside its image by `desc_score_key` (pk_common.h); ranks are a permutation, so every kept slot has exactly one writer
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const uint64_t kj = desc_score_key(dt_score[d0 + j]);
        int r = 0;
        for (int q = 0; q < n; ++q) {
            const uint64_t kq = desc_score_key(dt_score[d0 + q]);
            r += (kq < kj) || (kq == kj && q < j);
        }
        if (r < D) {
            sel[r] = d0 + j;
            cap_idx[cap_off[img] + r] = d0 + j;
        }
    }
    __syncthreads();
    const double eps = 2.220446049250313e-16;       // np.spacing(1)
    double* out = oks + oks_off[img];
    for (int p = threadIdx.x; p < D * G; p += blockDim.x) {
        const int d = p / G, g = p - d * G;
        const double* gk = gt_kpt + (size_t)(g0 + g) * K * 3;
        const double* dk = dt_kpt + (size_t)sel[d] * K * 3;
        int k1 = 0;
        for (int k = 0; k < K; ++k) k1 += gk[3 * k + 2] > 0;
        const double* bb = gt_bbox + (size_t)(g0 + g) * 4;
        const double x0 = bb[0] - bb[2], x1 = bb[0] + bb[2] * 2, y0 = bb[1] - bb[3], y1 = bb[1] + bb[3] * 2;
        const double aeps = gt_area[g0 + g] + eps;
        NpSum sum(k1 > 0 ? k1 : K);
        for (int k = 0; k < K; ++k) {
            if (k1 > 0 && !(gk[3 * k + 2] > 0)) continue;
            const double xd = dk[3 * k], yd = dk[3 * k + 1];
            double dx, dy;
            if (k1 > 0) {
                dx = xd - gk[3 * k];
                dy = yd - gk[3 * k + 1];
            } else {          // np.max((z, v), axis=0): NaN propagates
                const double ax = x0 - xd, bx = xd - x1, ay = y0 - yd, by = yd - y1;
                dx = (isnan(ax) || ax > 0 ? ax : 0.0) + (isnan(bx) || bx > 0 ? bx : 0.0);
                dy = (isnan(ay) || ay > 0 ? ay : 0.0) + (isnan(by) || by > 0 ? by : 0.0);
            }
            const double e = (dx * dx + dy * dy) / svar[k] / aeps / 2.0;
            sum.add(exp(-e));
        }
        out[p] = sum.total() / (double)(k1 > 0 ? k1 : K);
    }
}

// ---- evaluateImg: one lane per (area range a, threshold t), lane = a * T + t -------------------------------------------------------
// gt_flags: bit 0 ignore (iscrowd or num_keypoints == 0), bit 1 iscrowd.  Outputs per capped slot s and curve c: dt_match[c * n_cap + s] =
// index of the matched ground truth inside its image (file order) or -1, dt_ignore likewise; npig[img * A + a] = non-ignored ground truths.
__global__ void __launch_bounds__(64) k_coco_match(const double* __restrict__ oks, const int64_t* __restrict__ oks_off,
                                                   const int32_t* __restrict__ gt_off, const double* __restrict__ gt_area,
                                                   const int32_t* __restrict__ gt_flags, const int32_t* __restrict__ cap_off,
                                                   const int32_t* __restrict__ cap_idx, const double* __restrict__ dt_area,
                                                   const double* __restrict__ area_rng, const double* __restrict__ iou_thrs,
                                                   int32_t* __restrict__ dt_match, uint8_t* __restrict__ dt_ignore, int32_t* __restrict__ npig,
                                                   uint8_t* __restrict__ gtm_ws, int n_cap, int A, int T) {
    __shared__ uint8_t gtm_lds[PK_COCO_MAX_CURVES * PK_COCO_GTM_LDS];
    const int img = blockIdx.x, lane = threadIdx.x;
    if (lane >= A * T) return;
    const int g0 = gt_off[img], G = gt_off[img + 1] - g0;
    const int s0 = cap_off[img], D = cap_off[img + 1] - s0;
    const int a = lane / T, t = lane - a * T;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    // this lane's "already matched" flags (gtm[t, :] of evaluateImg for this area): only this lane reads and writes them
    uint8_t* gtm = (G <= PK_COCO_GTM_LDS ? gtm_lds + lane * PK_COCO_GTM_LDS : gtm_ws + (size_t)g0 * A * T + (size_t)lane * G);
    int nonign = 0;
    for (int g = 0; g < G; ++g) {
        gtm[g] = 0;
        const double ar = gt_area[g0 + g];
        nonign += !((gt_flags[g0 + g] & 1) || ar < lo || ar > hi);
    }
    if (t == 0) npig[img * A + a] = nonign;
    const double thr = fmin(iou_thrs[t], 1.0 - 1e-10);
    const double* o = oks + oks_off[img];
    for (int d = 0; d < D; ++d) {
        double best = thr;
        int m = -1, m_ign = 0;
        // ground truths stable-sorted by _ignore: the non-ignored ones (pass 0), then the ignored ones (pass 1); evaluateImg breaks at
        // the first ignored one once it holds a non-ignored match
        for (int pass = 0; pass < 2 && !(pass == 1 && m >= 0); ++pass)
            for (int g = 0; g < G; ++g) {
                const int fl = gt_flags[g0 + g];
                const double ar = gt_area[g0 + g];
                const int ign = (fl & 1) || ar < lo || ar > hi;
                if (ign != pass) continue;
                if (gtm[g] && !(fl & 2)) continue;
                const double v = o[(size_t)d * G + g];
                if (v < best) continue;
                best = v;
                m = g;
                m_ign = ign;
            }
        const size_t idx = (size_t)lane * n_cap + s0 + d;
        if (m >= 0) {
            gtm[m] = 1;
            dt_match[idx] = m;
            dt_ignore[idx] = (uint8_t)m_ign;
        } else {
            const double ar = dt_area[cap_idx[s0 + d]];
            dt_match[idx] = -1;
            dt_ignore[idx] = (uint8_t)(ar < lo || ar > hi);
        }
    }
}

// ---- accumulate's global order: order[rank] = slot, rank = stable rank by (-score, slot) --------------------------------------------
__global__ void __launch_bounds__(256) k_coco_rank(const double* __restrict__ dt_score, const int32_t* __restrict__ cap_idx,
                                                   int32_t* __restrict__ order, int n_cap) {
    __shared__ uint64_t tile[256];
    const int s = blockIdx.x * 256 + threadIdx.x;
    const uint64_t ks = s < n_cap ? desc_score_key(dt_score[cap_idx[s]]) : 0;
    int r = 0;
    for (int base = 0; base < n_cap; base += 256) {
        __syncthreads();
        if (base + (int)threadIdx.x < n_cap) tile[threadIdx.x] = desc_score_key(dt_score[cap_idx[base + threadIdx.x]]);
        __syncthreads();
        const int nt = min(256, n_cap - base);
        for (int q = 0; q < nt; ++q) {
            const uint64_t kq = tile[q];
            r += (kq < ks) || (kq == ks && base + q < s);
        }
    }
    if (s < n_cap) order[r] = s;
}

// ---- accumulate: one workgroup per curve c = a * T + t ---------------------------------------------------------------------------------
#define PK_COCO_ACC_THREADS 256
#define PK_COCO_ACC_ITEMS 16
// exclusive scan (sum) of one int per thread; returns the block total through *total
__device__ __forceinline__ int block_exclusive_sum(int v, int* sh, int* total) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < PK_COCO_ACC_THREADS; o <<= 1) {
        const int x = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += x;
        __syncthreads();
    }
    *total = sh[PK_COCO_ACC_THREADS - 1];
    return sh[tid] - v;
}

__global__ void __launch_bounds__(PK_COCO_ACC_THREADS) k_coco_accum(const int32_t* __restrict__ dt_match, const uint8_t* __restrict__ dt_ignore,
                                                                    const int32_t* __restrict__ npig_img, const int32_t* __restrict__ order,
                                                                    const double* __restrict__ rec_thrs, double* __restrict__ ws_pr,
                                                                    int32_t* __restrict__ ws_tp, double* __restrict__ precision,
                                                                    double* __restrict__ recall, int n_img, int n_cap, int A, int T, int R) {
    __shared__ int shi[PK_COCO_ACC_THREADS];
    __shared__ double shd[PK_COCO_ACC_THREADS];
    const int c = blockIdx.x, a = c / T, t = c - a * T, tid = threadIdx.x;
    int part = 0;
    for (int i = tid; i < n_img; i += PK_COCO_ACC_THREADS) part += npig_img[i * A + a];
    int npig;
    block_exclusive_sum(part, shi, &npig);
    if (npig == 0) {          // COCOeval leaves the -1 of its initialisation
        for (int r = tid; r < R; r += PK_COCO_ACC_THREADS) precision[((size_t)t * R + r) * A + a] = -1.0;
        if (tid == 0) recall[t * A + a] = -1.0;
        return;
    }
    const int32_t* mt = dt_match + (size_t)c * n_cap;
    const uint8_t* ig = dt_ignore + (size_t)c * n_cap;
    double* pr = ws_pr + (size_t)c * n_cap;
    int32_t* tpc = ws_tp + (size_t)c * n_cap;
    const double eps = 2.220446049250313e-16, dnp = (double)npig;
    const int CH = PK_COCO_ACC_THREADS * PK_COCO_ACC_ITEMS;
    // forward: tp / fp cumulative sums in ranked order, pr = tp / (fp + tp + eps)
    int carry_tp = 0, carry_fp = 0;
    for (int base = 0; base < n_cap; base += CH) {
        const int j0 = base + tid * PK_COCO_ACC_ITEMS, j1 = min(j0 + PK_COCO_ACC_ITEMS, n_cap);
        int ltp = 0, lfp = 0;
        for (int j = j0; j < j1; ++j) {
            const int s = order[j];
            if (!ig[s]) (mt[s] >= 0 ? ltp : lfp) += 1;
        }
        int tot_tp, tot_fp;
        int tp = carry_tp + block_exclusive_sum(ltp, shi, &tot_tp);
        int fp = carry_fp + block_exclusive_sum(lfp, shi, &tot_fp);
        for (int j = j0; j < j1; ++j) {
            const int s = order[j];
            if (!ig[s]) (mt[s] >= 0 ? tp : fp) += 1;
            tpc[j] = tp;
            pr[j] = (double)tp / (((double)fp + (double)tp) + eps);
        }
        carry_tp += tot_tp;
        carry_fp += tot_fp;
    }
    // backward: pr[i-1] = max(pr[i-1], pr[i]) from the end (suffix max; max is exact, so the scan order does not matter)
    double carry = -INFINITY;
    const int nch = (n_cap + CH - 1) / CH;
    for (int ci = nch - 1; ci >= 0; --ci) {
        __syncthreads();
        const int j0 = ci * CH + tid * PK_COCO_ACC_ITEMS, j1 = min(j0 + PK_COCO_ACC_ITEMS, n_cap);
        double lm = -INFINITY;
        for (int j = j0; j < j1; ++j) lm = fmax(lm, pr[j]);
        shd[tid] = lm;
        __syncthreads();
        for (int o = 1; o < PK_COCO_ACC_THREADS; o <<= 1) {      // inclusive suffix max over threads
            const double x = tid + o < PK_COCO_ACC_THREADS ? shd[tid + o] : -INFINITY;
            __syncthreads();
            shd[tid] = fmax(shd[tid], x);
            __syncthreads();
        }
        double run = fmax(carry, tid + 1 < PK_COCO_ACC_THREADS ? shd[tid + 1] : -INFINITY);
        for (int j = j1 - 1; j >= j0; --j) {
            run = fmax(run, pr[j]);
            pr[j] = run;
        }
        carry = fmax(carry, shd[0]);
    }
    __syncthreads();
    // q[r] = envelope[searchsorted(rc, recThrs[r], 'left')], 0 past the end; rc = tp / npig
    for (int r = tid; r < R; r += PK_COCO_ACC_THREADS) {
        const double v = rec_thrs[r];
        int lo = 0, hi = n_cap;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)tpc[mid] / dnp < v) lo = mid + 1;
            else hi = mid;
        }
        precision[((size_t)t * R + r) * A + a] = lo < n_cap ? pr[lo] : 0.0;
    }
    if (tid == 0) recall[t * A + a] = (double)tpc[n_cap - 1] / dnp;
}

// ---- C-ABI -------------------------------------------------------------------------------------------------------------------------
extern "C" int pk_coco_kpt_oks(const double* gt_kpt, const double* gt_bbox, const double* gt_area, const int32_t* gt_off, const double* dt_kpt,
                               const double* dt_score, const int32_t* dt_off, const double* vars, const int32_t* cap_off, const int64_t* oks_off,
                               int32_t* cap_idx, double* oks, int n_img, int K, int max_dets, void* stream) {
    PK_REQUIRE(gt_kpt && gt_bbox && gt_area && gt_off && dt_kpt && dt_score && dt_off && vars && cap_off && oks_off && cap_idx && oks,
               "pk_coco_kpt_oks: null pointer");
    PK_REQUIRE(n_img > 0 && K > 0 && max_dets > 0, "pk_coco_kpt_oks: bad size (n_img %d, K %d, max_dets %d)", n_img, K, max_dets);
    PK_SUPPORTED(K <= PK_COCO_MAX_K && max_dets <= PK_COCO_MAX_DETS, "pk_coco_kpt_oks: built for K <= %d and max_dets <= %d (got %d, %d)",
                 PK_COCO_MAX_K, PK_COCO_MAX_DETS, K, max_dets);
    hipLaunchKernelGGL(k_coco_oks, dim3(n_img), dim3(256), 0, (hipStream_t)stream, gt_kpt, gt_bbox, gt_area, gt_off, dt_kpt, dt_score, dt_off,
                       vars, cap_off, oks_off, cap_idx, oks, K, max_dets);
    return pk_launch_status("pk_coco_kpt_oks");
}

extern "C" int pk_coco_kpt_eval_ws_floats(int n_gt, int n_cap, int A, int T) {
    if (n_gt < 0 || n_cap < 0 || A < 0 || T < 0) return 0;
    const long long curves = (long long)A * T;
    const long long bytes = (curves * n_gt + 7) / 8 * 8 + curves * n_cap * 12;   // gtm overflow flags + (pr f64, tp i32) per curve and slot
    return (int)((bytes + 15) / 16 * 4);
}

extern "C" int pk_coco_kpt_eval(const double* oks, const int64_t* oks_off, const int32_t* gt_off, const double* gt_area, const int32_t* gt_flags,
                                const int32_t* cap_off, const int32_t* cap_idx, const double* dt_score, const double* dt_area,
                                const double* area_rng, const double* iou_thrs, const double* rec_thrs, int32_t* dt_match, uint8_t* dt_ignore,
                                int32_t* npig, int32_t* order, void* ws, double* precision, double* recall, int n_img, int n_gt, int n_cap,
                                int A, int T, int R, void* stream) {
    PK_REQUIRE(oks && oks_off && gt_off && gt_area && gt_flags && cap_off && cap_idx && dt_score && dt_area && area_rng && iou_thrs && rec_thrs &&
               dt_match && dt_ignore && npig && order && ws && precision && recall, "pk_coco_kpt_eval: null pointer");
    PK_REQUIRE(n_img > 0 && n_gt > 0 && n_cap > 0 && A > 0 && T > 0 && R > 0,
               "pk_coco_kpt_eval: bad size (n_img %d, n_gt %d, n_cap %d, A %d, T %d, R %d)", n_img, n_gt, n_cap, A, T, R);
    PK_SUPPORTED(A * T <= PK_COCO_MAX_CURVES, "pk_coco_kpt_eval: built for A * T <= %d curves (got %d)", PK_COCO_MAX_CURVES, A * T);
    const long long curves = (long long)A * T;
    uint8_t* gtm_ws = (uint8_t*)ws;
    const size_t pr_off = (size_t)((curves * n_gt + 7) / 8 * 8);
    double* ws_pr = (double*)((uint8_t*)ws + pr_off);
    int32_t* ws_tp = (int32_t*)(ws_pr + curves * n_cap);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_coco_match, dim3(n_img), dim3(64), 0, st, oks, oks_off, gt_off, gt_area, gt_flags, cap_off, cap_idx, dt_area, area_rng,
                       iou_thrs, dt_match, dt_ignore, npig, gtm_ws, n_cap, A, T);
    int rc = pk_launch_status("pk_coco_kpt_eval (match)");
    if (rc) return rc;
    hipLaunchKernelGGL(k_coco_rank, dim3((n_cap + 255) / 256), dim3(256), 0, st, dt_score, cap_idx, order, n_cap);
    if ((rc = pk_launch_status("pk_coco_kpt_eval (rank)"))) return rc;
    hipLaunchKernelGGL(k_coco_accum, dim3(A * T), dim3(PK_COCO_ACC_THREADS), 0, st, dt_match, dt_ignore, npig, order, rec_thrs, ws_pr, ws_tp,
                       precision, recall, n_img, n_cap, A, T, R);
    return pk_launch_status("pk_coco_kpt_eval (accumulate)");
}

// ================================================================================================ f1: evaluator records
// COCOEvaluator.update (utils/metrics.py:84-106): per instance a (K,3) array [x, y, score] and the instance score = mean of the
// strictly positive keypoint scores (0 when there is none).  One 64-lane wave per instance; the mean is an fp32 sum in keypoint
// order divided by the count (numpy's float32 mean sums pairwise: equal to 1e-6 relative, stated in the test).
__global__ void __launch_bounds__(64) k_pose_records(const float* __restrict__ kp, const float* __restrict__ sc, float* __restrict__ rec,
                                                    float* __restrict__ inst, int K) {
    const int b = blockIdx.x, t = threadIdx.x;
    for (int k = t; k < K; k += 64) {
        rec[((size_t)b * K + k) * 3 + 0] = kp[((size_t)b * K + k) * 2 + 0];
        rec[((size_t)b * K + k) * 3 + 1] = kp[((size_t)b * K + k) * 2 + 1];
        rec[((size_t)b * K + k) * 3 + 2] = sc[(size_t)b * K + k];
    }
    if (t == 0) {
        float s = 0.f;
        int n = 0;
        for (int k = 0; k < K; ++k) {
            const float v = sc[(size_t)b * K + k];
            if (v > 0.f) {
                s += v;
                ++n;
            }
        }
        inst[b] = n > 0 ? s / (float)n : 0.f;
    }
}
extern "C" int pk_pose_records(const float* keypoints, const float* scores, float* records, float* instance_score, int B, int K,
                               void* stream) {
    PK_REQUIRE(keypoints && scores && records && instance_score && B > 0 && K > 0, "pk_pose_records: bad argument");
    hipLaunchKernelGGL(k_pose_records, dim3(B), dim3(64), 0, (hipStream_t)stream, keypoints, scores, records, instance_score, K);
    return pk_launch_status("pk_pose_records");
}
