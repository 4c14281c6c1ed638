// Detector-box validation on the device: pose rescoring and OKS-NMS (hard and soft) of the poses of every image (DESIGN section 4,
// "Detector boxes and OKS-NMS").  The semantics are this project's specification (include/posekernels.h); the reference names the
// protocol in its yaml (TEST.USE_GT_BBOX: false) and implements none of it.
//
//   k_pose_rescore   one thread per pose: box score x mean of the keypoint scores above in_vis_thr, summed over k ascending
//   k_oks_nms        one workgroup per image: the greedy suppression is a data-dependent chain inside an image (whether pose i is visited
//                    depends on every earlier visit) and independent across images, so the chain runs serially in one workgroup and the
//                    work of one link -- the OKS of the selected pose to every later / remaining pose -- is spread over its threads
// Everything fp64.  No atomics: every LDS word has one writer between two barriers, every floating-point value is computed by one thread
// in a fixed order, and every output element is written once, at the end, by one thread -- two launches give identical bytes.
#include "pk_common.h"

#include <math.h>

#define PK_NMS_THREADS 256      // one workgroup per image; its PK_NMS_MAX_POSES scores, flags and ranks live in LDS

__global__ void __launch_bounds__(256) k_pose_rescore(const double* __restrict__ kpt, const double* __restrict__ box_score,
                                                      double* __restrict__ score_out, int N, int K, double in_vis_thr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double* p = kpt + (size_t)i * K * 3;
    double sum = 0.0;
    int cnt = 0;
    for (int k = 0; k < K; ++k) {
        const double s = p[3 * k + 2];
        if (s > in_vis_thr) {
            sum += s;
            ++cnt;
        }
    }
    const double mean = cnt > 0 ? sum / (double)cnt : 0.0;
    score_out[i] = (box_score ? box_score[i] : 1.0) * mean;
}

// OKS of the selected pose (keypoints staged in LDS) and pose c of the same image.  Joint k counts when both keypoint scores exceed
// in_vis_thr; 0 without such a joint.
__device__ __forceinline__ double pair_oks(const double* __restrict__ a, double area_a, const double* __restrict__ b, double area_b,
                                           const double* __restrict__ svar, int K, double in_vis_thr) {
    const double denom = (area_a + area_b) / 2.0 + 2.220446049250313e-16;
    double sum = 0.0;
    int cnt = 0;
    for (int k = 0; k < K; ++k) {
        if (!(a[3 * k + 2] > in_vis_thr && b[3 * k + 2] > in_vis_thr)) continue;
        const double dx = a[3 * k] - b[3 * k], dy = a[3 * k + 1] - b[3 * k + 1];
        const double e = (dx * dx + dy * dy) / svar[k] / denom / 2.0;
        sum += exp(-e);
        ++cnt;
    }
    return cnt > 0 ? sum / (double)cnt : 0.0;
}

__global__ void __launch_bounds__(PK_NMS_THREADS) k_oks_nms(const double* __restrict__ kpt, const double* __restrict__ area,
                                                            const double* __restrict__ score, const int32_t* __restrict__ off,
                                                            const double* __restrict__ vars, uint8_t* __restrict__ keep,
                                                            int32_t* __restrict__ n_keep, int32_t* __restrict__ order,
                                                            double* __restrict__ out_score, int K, double thr, double in_vis_thr, int soft,
                                                            int max_dets) {
    __shared__ double cur[PK_NMS_MAX_POSES];          // current score of every pose (hard mode: the input score)
    __shared__ int sorted[PK_NMS_MAX_POSES];          // hard mode: local index of each rank
    __shared__ int ord[PK_NMS_MAX_POSES];             // kept local indices in selection order
    __shared__ uint8_t alive[PK_NMS_MAX_POSES];       // not yet removed (hard) / not yet selected (soft)
    __shared__ uint8_t kept[PK_NMS_MAX_POSES];
    __shared__ double svar[PK_NMS_MAX_K];
    __shared__ double sel_kpt[PK_NMS_MAX_K * 3];      // keypoints of the pose selected in this link of the chain
    __shared__ uint64_t red_key[PK_NMS_THREADS];
    __shared__ int red_idx[PK_NMS_THREADS];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int d0 = off[img], n = off[img + 1] - d0;
    if (n <= 0 || n > PK_NMS_MAX_POSES) {             // no poses: nothing to write but the count; beyond the LDS arrays: refused (-1), the
        if (tid == 0) n_keep[img] = n <= 0 ? 0 : -1;  // host wrapper checks the offsets before it launches
        return;
    }
    for (int k = tid; k < K; k += PK_NMS_THREADS) svar[k] = vars[k];
    for (int j = tid; j < n; j += PK_NMS_THREADS) {
        cur[j] = score[d0 + j];
        alive[j] = 1;
        kept[j] = 0;
    }
    __syncthreads();
    const double* kp0 = kpt + (size_t)d0 * K * 3;
    int cnt = 0;                                      // the same value in every thread
    if (!soft) {
        // stable rank by descending score (`desc_score_key`, ties to the lower index); the ranks are a permutation, so every slot of
        // sorted[] has exactly one writer
        for (int j = tid; j < n; j += PK_NMS_THREADS) {
            const uint64_t kj = desc_score_key(cur[j]);
            int r = 0;
            for (int q = 0; q < n; ++q) {
                const uint64_t kq = desc_score_key(cur[q]);
                r += (kq < kj) || (kq == kj && q < j);
            }
            sorted[r] = j;
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const int p = sorted[i];
            if (!alive[p]) continue;                  // uniform: alive[] was last written before the barrier that ended the previous link
            for (int t = tid; t < 3 * K; t += PK_NMS_THREADS) sel_kpt[t] = kp0[(size_t)p * K * 3 + t];
            if (tid == 0) {
                ord[cnt] = p;
                kept[p] = 1;
            }
            ++cnt;
            __syncthreads();
            const double area_p = area[d0 + p];
            for (int t = i + 1 + tid; t < n; t += PK_NMS_THREADS) {
                const int c = sorted[t];
                if (!alive[c]) continue;
                const double o = pair_oks(sel_kpt, area_p, kp0 + (size_t)c * K * 3, area[d0 + c], svar, K, in_vis_thr);
                if (o > thr) alive[c] = 0;
            }
            __syncthreads();
        }
    } else {
        const int want = min(n, max_dets);
        while (cnt < want) {
            // the remaining pose with the highest current score, ties to the lower index: lexicographic minimum of (key, index)
            uint64_t bk = ~0ull;
            int bi = 0x7fffffff;
            for (int j = tid; j < n; j += PK_NMS_THREADS) {
                if (!alive[j]) continue;
                const uint64_t kj = desc_score_key(cur[j]);
                if (kj < bk || (kj == bk && j < bi)) {
                    bk = kj;
                    bi = j;
                }
            }
            red_key[tid] = bk;
            red_idx[tid] = bi;
            __syncthreads();
            for (int o = PK_NMS_THREADS / 2; o > 0; o >>= 1) {
                if (tid < o) {
                    const uint64_t k2 = red_key[tid + o];
                    const int i2 = red_idx[tid + o];
                    if (k2 < red_key[tid] || (k2 == red_key[tid] && i2 < red_idx[tid])) {
                        red_key[tid] = k2;
                        red_idx[tid] = i2;
                    }
                }
                __syncthreads();
            }
            const int p = red_idx[0];                 // cnt < n poses are selected, so one remains: p is a valid index
            for (int t = tid; t < 3 * K; t += PK_NMS_THREADS) sel_kpt[t] = kp0[(size_t)p * K * 3 + t];
            if (tid == 0) {
                ord[cnt] = p;
                kept[p] = 1;
                alive[p] = 0;
            }
            ++cnt;
            __syncthreads();                          // also: every thread has read red_idx[0] before the next reduction overwrites it
            const double area_p = area[d0 + p];
            for (int c = tid; c < n; c += PK_NMS_THREADS) {
                if (!alive[c]) continue;
                const double o = pair_oks(sel_kpt, area_p, kp0 + (size_t)c * K * 3, area[d0 + c], svar, K, in_vis_thr);
                cur[c] = cur[c] * exp(-(o * o) / thr);
            }
            __syncthreads();
        }
    }
    // ord[] and kept[] were last written before a barrier
    for (int j = tid; j < n; j += PK_NMS_THREADS) {
        keep[d0 + j] = kept[j];
        order[d0 + j] = j < cnt ? ord[j] : -1;
        out_score[d0 + j] = kept[j] ? cur[j] : 0.0;   // a selected pose left the remaining set: its score stayed as it was at selection
    }
    if (tid == 0) n_keep[img] = cnt;
}

// ---- C-ABI -------------------------------------------------------------------------------------------------------------------------
extern "C" int pk_pose_rescore(const double* kpt, const double* box_score, double* score_out, int N, int K, double in_vis_thr, void* stream) {
    PK_REQUIRE(kpt && score_out, "pk_pose_rescore: null pointer");
    PK_REQUIRE(N > 0 && K > 0 && K <= PK_NMS_MAX_K, "pk_pose_rescore: bad size (N %d, K %d; 1 <= K <= %d)", N, K, PK_NMS_MAX_K);
    PK_REQUIRE(!isnan(in_vis_thr), "pk_pose_rescore: in_vis_thr is NaN");
    hipLaunchKernelGGL(k_pose_rescore, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, kpt, box_score, score_out, N, K, in_vis_thr);
    return pk_launch_status("pk_pose_rescore");
}

extern "C" int pk_oks_nms(const double* kpt, const double* area, const double* score, const int32_t* off, const double* vars, uint8_t* keep,
                          int32_t* n_keep, int32_t* order, double* out_score, int n_img, int K, double thr, double in_vis_thr, int soft,
                          int max_dets, void* stream) {
    PK_REQUIRE(kpt && area && score && off && vars && keep && n_keep && order && out_score, "pk_oks_nms: null pointer");
    PK_REQUIRE(n_img > 0 && K > 0 && K <= PK_NMS_MAX_K, "pk_oks_nms: bad size (n_img %d, K %d; 1 <= K <= %d)", n_img, K, PK_NMS_MAX_K);
    PK_REQUIRE(isfinite(thr) && !isnan(in_vis_thr), "pk_oks_nms: thr must be finite and in_vis_thr a number (got %g, %g)", thr, in_vis_thr);
    PK_REQUIRE(!soft || (thr > 0.0 && max_dets > 0), "pk_oks_nms: soft mode needs thr > 0 and max_dets > 0 (got %g, %d)", thr, max_dets);
    hipLaunchKernelGGL(k_oks_nms, dim3(n_img), dim3(PK_NMS_THREADS), 0, (hipStream_t)stream, kpt, area, score, off, vars, keep, n_keep, order,
                       out_score, K, thr, in_vis_thr, soft, max_dets);
    return pk_launch_status("pk_oks_nms");
}
