/* libposekernels — C-ABI of the MI355X (gfx950) pose-estimation hot path.
 *
 * The reference (MarkJhonBao/InfantPoseEstimation_GaussianBias) is pure Python/PyTorch and has NO
 * FFI/plugin boundary of its own; the Python class/function surface is its interface.
 * This header is therefore the boundary this build defines underneath that surface: every entry point
 * replaces one group of ATen calls made by a reference function, cited as (file:line) below.
 *
 * Conventions (all entries):
 *   - extern "C", plain pointers and sizes; no C++/torch types.
 *   - every pointer is a BORROWED DEVICE pointer (caller allocates inputs, outputs and workspaces);
 *     the library allocates nothing and keeps no state besides a thread-local error string.  It reads seven environment
 *     switches, per call, that route convolutions to / away from the specialised kernels (PK_CONV8P, PK_CONV8P_MIN_TILES,
 *     PK_CONV3H, PK_CONV3H_MIN_TILES, PK_CONV1X1_BN, PK_CONV1X1_BN_MIN_ROWS, PK_CONV1X1_BN_MAX_GRID: used by the parity tests to push
 *     small shapes through them) and nothing else.
 *   - asynchronous on `stream` (a hipStream_t passed as void*); no internal synchronisation; graph-capturable.
 *   - returns 0 on success, a negative PK_ERR_* on argument validation failure (nothing launched),
 *     or a positive hipError_t from the launch.  Never throws, never aborts.
 *   - layouts: "maps" are (B,K,H,W) fp32 contiguous; features are NHWC; bf16 is the 16-bit upper half of fp32.
 */
#ifndef POSEKERNELS_H
#define POSEKERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PK_OK 0
#define PK_ERR_INVALID (-1)     /* bad shape / null pointer / misalignment */
#define PK_ERR_UNSUPPORTED (-2) /* shape outside what the kernels are built for */

#define PK_DT_F32 0
#define PK_DT_BF16 1

int pk_version(void);                      /* 10000*major + 100*minor + patch */
const char* pk_last_error_string(void);    /* thread-local; valid until the next failing call on this thread */
int pk_marker(int id, void* stream);       /* profiling aid: empty launch of `id` workgroups that cuts a kernel trace into sections */

/* ---- T1: COCOPoseDataset._generate_target (datasets/coco_dataset.py:185-250), batched ------------------
 * keypoints (B,K,2) f32 input-px; visible (B,K) f32 (COCO v: 0/1/2); lut = host-built patch values indexed
 * by integer d2=dx^2+dy^2 (lut_len entries; built with the reference's own float32 numpy expression so the
 * result is bit-exact); patch side n, centre c; reach = 3*sigma; stride = input/heatmap size (double).
 * Writes EVERY element of target (B,K,Hh,Wh) and weight (B,K,1).                                          */
int pk_gaussian_target(const float* keypoints, const float* visible, const float* lut, int lut_len,
                       float* target, float* weight, int B, int K, int Hh, int Wh,
                       double stride_x, double stride_y, double reach, int patch_n, int patch_c, void* stream);

/* ---- T2: GenerateTarget (data/pose_transforms.py:385-457): dense sub-pixel Gaussian, weight 0/1 -------- */
int pk_dense_target(const float* keypoints, const float* visible, float* heatmaps, float* weights,
                    int B, int K, int Hh, int Wh, float scale_x, float scale_y, float sigma, void* stream);

/* ---- D2/D3: argmax decoders.  mode 0: get_max_preds (utils/postprocess.py:10-34); mode 1: quarter shift of
 * PoseEstimator.decode_heatmaps (models/pose_estimator.py:331-373); mode 2: Taylor sub-pixel of
 * get_max_preds_with_subpixel (utils/postprocess.py:37-75).  index: first maximum (ties -> lowest index).    */
int pk_argmax_decode(const float* heatmaps, int32_t* index, float* maxval, float* coords,
                     int BK, int H, int W, int mode, void* stream);

/* ---- Unbiased (distribution-aware, "DARK") decode: this project's own specification (DESIGN.md "Unbiased decoding"; the reference names
 * TEST.POST_PROCESS in its yamls and implements nothing beyond modes 1 and 2 above).  One workgroup per map; NaN counts as the maximum and
 * ties go to the lowest flat index, as in pk_argmax_decode.  taps_host: HOST pointer to ksize floats (odd, 3 .. 31), read before the call
 * returns and carried in the kernel's arguments (no device table, no allocation: graph-capturable).  index (BK) int32, maxval (BK) and
 * refined (BK) uint8 may be NULL; coords (BK,2) may not.  The published form blurs the whole map and rescales it to the raw maximum
 * before the logarithm; that rescale adds a constant to the log map and cancels in every difference below, so it is dropped, and only
 * the 13 stencil points need the blur: every heatmap element is read from global memory once (the argmax), then a (ksize + 4) x 5 patch is
 * blurred.  All float32, one rounding per operation, in this order, with c = (ksize-1)/2 and m = 0 outside the map (zero padding):
 *   (px, py) = first maximum of m;  maxval = m[py][px];  index = py W + px;
 *   R[y][x] = sum_t g[t] m[y][x+t-c]:  acc = 0.0f, then acc = fmaf(g[t], v, acc) for t = 0 .. ksize-1;   B[y][x] = sum_t g[t] R[y+t-c][x], alike;
 *   L = logf(fmaxf(B, 1e-10f));   with L(j, i) = L[py+j][px+i]:
 *   dx = 0.5f (L(0,1) - L(0,-1));  dy = 0.5f (L(1,0) - L(-1,0));  dxx = 0.25f (L(0,2) - 2 L(0,0) + L(0,-2));  dyy = 0.25f (L(2,0) - 2 L(0,0) + L(-2,0));
 *   dxy = 0.25f (L(1,1) - L(-1,1) - L(1,-1) + L(-1,-1));   det = dxx dyy - dxy dxy;   ox = -(dyy dx - dxy dy) / det;   oy = -(dxx dy - dxy dx) / det.
 * The step is taken iff 2 <= px <= W-3 and 2 <= py <= H-3, dxx < 0 and det > 0 (a maximum), |ox| <= 2 and |oy| <= 2 (the reach of the
 * stencil) -- positive comparisons, which a NaN fails.  Then refined = 1 and coords = (px + ox, py + oy); otherwise refined = 0 and coords =
 * (px, py), exactly the integers (constant, all-zero and non-positive maps, NaN / inf maps, border peaks).  Two launches: identical bytes.
 * PK_ERR_INVALID, before any launch: null heatmaps / coords / taps_host, a ksize that is even or outside 3 .. 31, a bad shape.          */
int pk_unbiased_decode(const float* heatmaps, const float* taps_host, int ksize, int32_t* index, float* maxval, float* coords,
                       uint8_t* refined, int BK, int H, int W, void* stream);

/* ---- D1: HeatmapRegressionHead.decode (models/fusion_head.py:309-365) = SoftArgmax2D (:24-71) +
 * LocalGaussianRefinement (:74-128) + alpha blend (:169-170) + offset sampling.  alpha/fusion_weight are the
 * RAW parameters (sigmoid applied inside), read from device memory.  offsets may be NULL (apply_offset=False). */
int pk_softargmax_refine_decode(const float* heatmaps, const float* offsets, const float* alpha_param,
                                const float* fusion_weight_param, float* coords, float* scores,
                                int BK, int H, int W, int local_radius, void* stream);

/* ---- D3 remainder (utils/postprocess.py:78-184,226-238,270-292) on (B,K,2) coordinates ----------------- */
int pk_window_refine(const float* heatmaps, const float* coords_in, float* coords_out, int BK, int H, int W,
                     int window, void* stream);                                  /* coordinate_refinement */
int pk_fused_blend(const float* hp, const float* maxvals, const float* regression, float* out, int BK,
                   float sx, float sy, float reg_scale, void* stream);           /* fused_decode tail */
int pk_affine_coords(const float* coords, const float* center, const float* scale, float* out, int B, int K,
                     float mul_x, float mul_y, const float* mask_maxvals, float threshold, void* stream);
                     /* out = mask * coords * (scale*mul) + center - scale/2 : transform_preds / train.py:328-336 */

/* ---- f1: COCOEvaluator.update arrays (utils/metrics.py:84-106): records (B,K,3) = [x, y, score], instance_score (B) = mean of
 * the strictly positive keypoint scores (0 if none) ----------------------------------------------------------------------- */
int pk_pose_records(const float* keypoints, const float* scores, float* records, float* instance_score, int B, int K,
                    void* stream);

/* ---- f1: COCO keypoint AP/AR (COCOeval iouType='keypoints', one category, one maxDets; utils/coco_eval.py holds the host side) --------
 * Everything fp64.  Images are the evaluated image ids in ascending order; ground truths and detections are grouped by image in CSR form
 * (gt_off, dt_off: n_img + 1 offsets; file / record order inside an image).  gt_kpt (G,K,3) with the visibility, gt_bbox (G,4) x y w h,
 * gt_area (G); dt_kpt (N,K,3) (only x, y read), dt_score (N); vars = (2 sigma)^2 (K).  cap_off[i] = sum of min(n_j, max_dets) over j < i,
 * oks_off[i] = sum of min(n_j, max_dets) * G_j.
 * pk_coco_kpt_oks (computeOks): per image, stable-ranks the detections by descending score (NaN last, ties in record order), keeps the
 *   first max_dets (cap_idx[cap_off[i] + r] = detection index of rank r) and writes the OKS block oks[oks_off[i] + r * G_i + g].
 *   K <= 64, max_dets <= 64.
 * pk_coco_kpt_eval (evaluateImg + accumulate): gt_flags bit 0 = ignore (iscrowd or num_keypoints == 0), bit 1 = iscrowd; dt_area (N);
 *   area_rng (A,2) inclusive; iou_thrs (T); rec_thrs (R); A * T <= 64.  Writes dt_match / dt_ignore (A*T, n_cap): matched ground truth
 *   (index inside its image, file order) or -1, and the ignore flag of each capped slot per curve a * T + t; npig (n_img, A): non-ignored
 *   ground truths; order (n_cap): capped slots by descending score, stable; precision (T,R,A) and recall (T,A) in COCOeval's
 *   eval['precision'][:, :, 0, :, 0] / eval['recall'][:, 0, :, 0] layout (-1 where an area has no non-ignored ground truth).
 *   ws: pk_coco_kpt_eval_ws_floats(n_gt, n_cap, A, T) floats.                                                                        */
int pk_coco_kpt_oks(const double* gt_kpt, const double* gt_bbox, const double* gt_area, const int32_t* gt_off, const double* dt_kpt,
                    const double* dt_score, const int32_t* dt_off, const double* vars, const int32_t* cap_off, const int64_t* oks_off,
                    int32_t* cap_idx, double* oks, int n_img, int K, int max_dets, void* stream);
int pk_coco_kpt_eval_ws_floats(int n_gt, int n_cap, int A, int T);
int pk_coco_kpt_eval(const double* oks, const int64_t* oks_off, const int32_t* gt_off, const double* gt_area, const int32_t* gt_flags,
                     const int32_t* cap_off, const int32_t* cap_idx, const double* dt_score, const double* dt_area, const double* area_rng,
                     const double* iou_thrs, const double* rec_thrs, int32_t* dt_match, uint8_t* dt_ignore, int32_t* npig, int32_t* order,
                     void* ws, double* precision, double* recall, int n_img, int n_gt, int n_cap, int A, int T, int R, void* stream);

/* ---- f1: validation on detector boxes: pose rescoring and OKS-NMS per image (this project's own specification, DESIGN.md "Detector boxes
 * and OKS-NMS": the reference's yaml says TEST.USE_GT_BBOX: false and its code has neither step).  Everything fp64; no atomics, fixed
 * orders: two launches give identical bytes.  Poses of all images in CSR form: off (n_img + 1) int32 offsets, kpt (N,K,3) rows
 * [x, y, keypoint score], area (N), score (N); vars = (2 sigma)^2 (K).  1 <= K <= PK_NMS_MAX_K (else PK_ERR_INVALID).
 * pk_pose_rescore: score_out[i] = box_score[i] * mean{ s_k : s_k > in_vis_thr }, the sum over k ascending, then one divide and one
 *   multiply; 0 when no joint qualifies; box_score == NULL means 1.  in_vis_thr may be -inf (every non-NaN score counts), not NaN.
 * pk_oks_nms: one workgroup per image.  Pose-pair OKS: joint k counts when both poses have a keypoint score > in_vis_thr;
 *   e_k = (dx^2 + dy^2) / vars_k / ((area_a + area_b) / 2 + 2.220446049250313e-16) / 2; oks = sum_k exp(-e_k) / count over k ascending, 0
 *   when no joint counts.
 *   soft == 0: poses are visited by descending score (ties to the lower index, NaN last: pk_coco_kpt_oks's rule); a visited pose that is
 *     still alive is kept and removes every later alive pose with oks > thr (strict).  max_dets is not read.
 *   soft != 0 (thr > 0, max_dets > 0): until max_dets poses are kept or none remains, the remaining pose with the highest current score
 *     (same ordering rule) is selected and every remaining score is multiplied by exp(-oks^2 / thr), oks taken to the selected pose.
 *   Outputs, every element of an image with poses written: keep (N) uint8; n_keep (n_img) int32; order (N) int32: per image its kept
 *   local indices in selection order, then -1; out_score (N): the input score (soft == 0) or the score at selection, 0 where not kept.
 *   At most PK_NMS_MAX_POSES poses per image.  The offsets are device memory, so the entry cannot read them: the caller checks them (hipops.oks_nms
 *   raises with PK_ERR_UNSUPPORTED, naming the image and its count, before anything is launched); a workgroup that meets more writes only
 *   n_keep = -1 for its image.  A non-finite thr, a NaN in_vis_thr and soft mode with thr <= 0 or max_dets <= 0 are PK_ERR_INVALID.      */
#define PK_NMS_MAX_K 64
#define PK_NMS_MAX_POSES 1024
int pk_pose_rescore(const double* kpt, const double* box_score, double* score_out, int N, int K, double in_vis_thr, void* stream);
int pk_oks_nms(const double* kpt, const double* area, const double* score, const int32_t* off, const double* vars, uint8_t* keep,
               int32_t* n_keep, int32_t* order, double* out_score, int n_img, int K, double thr, double in_vis_thr, int soft, int max_dets,
               void* stream);

/* ---- f2: input pipeline (datasets/transforms.py:42-47,128-131,212-217; datasets/coco_dataset.py:156-163; inference.py:83-110):
 * affine crop (OpenCV 8-bit warpAffine INTER_LINEAR / BORDER_CONSTANT 0 integer algorithm, see oracle/warp.py; parity unpinned vs cv2
 * itself) + optional column mirror + optional BGR->RGB + ((v/255) - mean)/std, whole batch, one launch.  src_u8: device buffer holding the
 * decoded (H,W,3) uint8 images; desc_table rows (72 bytes): { int64 src_offset; int32 H, W, flip, bgr; double minv[6] } with minv the
 * INVERSE (destination->source) matrix in float64; mean3/std3 are HOST pointers (read before the launch returns).  Outputs (either may be
 * NULL): fp32 NCHW (B,3,out_h,out_w) -- the reference's batch['img'] -- and bf16 NHWC with 8-channel pixels (B,out_h,out_w,8), the stem
 * convolution's input layout (channels 3..7 zero).                                                                                 */
int pk_affine_crop_normalize(const void* src_u8, const void* desc_table, int n_samples, int out_w, int out_h, float* out_nchw_f32,
                             void* out_nhwc8_bf16, const float* mean3, const float* std3, void* stream);
/* The same crop with the reference's CustomColorJitter (data/examples.py:367-401) between the 8-bit warp and the normalisation.
 * jitter_table rows (16 bytes): { int32 enable; float b, c, s } (brightness, contrast, saturation factors), one per sample.  With
 * u the crop's bytes, N = 3 out_w out_h and S their exact integer sum, every operation rounded once to float32 (no FMA):
 *   m = (float)((double)S / (255.0 N) * (double)b);   x = u / 255 * b;   x = (x - m) * c + m;   g = ((x0 + x1) + x2) / 3 per pixel;
 *   x = g + (x - g) * s;   u' = (int)(min(max(x, 0), 1) * 255);   then ((u' / 255) - mean) / std as above.
 * A row with enable == 0 gives exactly pk_affine_crop_normalize's output for that sample (factors 1, 1, 1 do not: the / 255 * 255
 * round trip truncates).  Two launches on `stream`; ws: pk_affine_crop_jitter_ws_bytes(n_samples, out_w, out_h) bytes, 4-byte aligned
 * (the query returns PK_ERR_INVALID for a refused shape: 765 out_w out_h must stay below 2^32).                                     */
int pk_affine_crop_jitter_ws_bytes(int n_samples, int out_w, int out_h);
int pk_affine_crop_jitter_normalize(const void* src_u8, const void* desc_table, const void* jitter_table, int n_samples, int out_w, int out_h,
                                    float* out_nchw_f32, void* out_nhwc8_bf16, const float* mean3, const float* std3, void* ws,
                                    int64_t ws_bytes, void* stream);
/* The same crop with this project's occlusion, blur and noise augmentation (DESIGN.md "Occlusion, blur and noise on the device") on the
 * warped bytes, per sample in this order: colour jitter (exactly the arithmetic above, m from the byte sum of the warped crop), Gaussian
 * blur, additive sensor noise, rectangle erasing, then the normalisation.  Every stage has an off state in which it does nothing: a row
 * with only the jitter on gives pk_affine_crop_jitter_normalize's bits, a row of zeros pk_affine_crop_normalize's.  Blur, noise and erasing
 * are integer arithmetic, with pix = y out_w + x and uint32 arithmetic mod 2^32 in
 *   hash(seed, pix, stream):  x = seed + pix 0x9E3779B9 + stream 0x85EBCA6B;  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *   blur (radius R = 1 .. PK_AUG_MAX_RADIUS, 0 = off; weights q[0] + 2 sum_{k>=1} q[k] = 256; clamp-to-edge), per channel:
 *     t(x, y) = (sum_{k=-R..R} q[|k|] u(clamp(x + k), y) + 128) >> 8;   v(x, y) = (sum_k q[|k|] t(x, clamp(y + k)) + 128) >> 8
 *   noise (amp = 1 .. 255, 0 = off), channel c:  h = hash(noise_seed, pix, 0x100 + c);  s = sum of the four bytes of h - 510;
 *     v' = clamp(v + ((amp s + 256) >> 9), 0, 255), the shift arithmetic (floor)
 *   erasing (n_rects = 0 .. PK_AUG_MAX_RECTS): rectangle r covers x0 <= x < x1, y0 <= y < y1 (clipped to the crop by that test; may be
 *     empty), a later one overwrites an earlier one; mode 0 writes its RGB bytes, mode 1 bytes 0, 1, 2 of hash(erase_seed, pix, 1 + r).
 * aug_table rows (PK_AUG_ROW_BYTES = 176 bytes, 16-byte aligned), one per sample, little-endian, in this order:
 *   int32 jitter_enable; float b, c, s;  int32 radius;  int32 q[8] (q[0] centre; entries beyond radius unread);  int32 amp;  uint32 noise_seed;
 *   int32 n_rects;  uint32 erase_seed;  4 x { int32 x0, y0, x1, y1;  int32 mode;  uint32 rgb = r | g << 8 | b << 16 };  12 bytes of padding.
 * The table is device memory, so the entry cannot check the rows: the caller does (DeviceCropper raises before anything is staged).  The
 * kernel clamps radius to 0 .. 7, amp to 0 .. 255 and n_rects to 0 .. 4, treats every mode but 0 as 1, and writes nothing out of bounds
 * whatever a row holds.  Two launches on `stream` (the warp into the workspace, then one 32 x 32 output tile per workgroup); ws:
 * pk_affine_crop_augment_ws_bytes(n_samples, out_w, out_h) bytes -- the jitter entry's formula and its 2^32 refusal -- 4-byte aligned.
 * PK_ERR_INVALID before any launch: a null pointer, a bad shape, a short workspace, a misaligned workspace, NHWC output or table.        */
#define PK_AUG_MAX_RADIUS 7
#define PK_AUG_MAX_RECTS 4
#define PK_AUG_ROW_BYTES 176
int pk_affine_crop_augment_ws_bytes(int n_samples, int out_w, int out_h);
int pk_affine_crop_augment_normalize(const void* src_u8, const void* desc_table, const void* aug_table, int n_samples, int out_w, int out_h,
                                     float* out_nchw_f32, void* out_nhwc8_bf16, const float* mean3, const float* std3, void* ws,
                                     int64_t ws_bytes, void* stream);

/* ---- D4: flip-test merge (models/pose_estimator.py:303-319): out = (a + swapLR(flipW(b)))/2 ------------- */
int pk_flip_merge(const float* a, const float* b_flipped, const int32_t* partner, float* out,
                  int B, int K, int H, int W, void* stream);

/* ---- D4 over several crop scales: multi-scale flip test (this project's own specification; the reference names the option in its yaml,
 * ADVANCED.MULTI_SCALE_TEST / SCALE_LIST, and never implemented it).  stack (S*F*B, K, H, W) fp32, pass-major: pass p = s*F + f holds
 * rows [p*B, (p+1)*B); f = 0 is the plain crop taken with box scale scale_s * scale around the same centre, f = 1 the forward of the
 * mirrored crop (F = 1 or 2, 1 <= S <= 8).  partner (K) int32 as for pk_flip_merge, may be NULL when F = 1.  inv_scales_host: HOST
 * pointer to S floats, entry s = (float)(1.0 / (double)scale_s), read before the call returns and carried in the kernel's arguments
 * (no device table, no allocation: graph-capturable).  out (B, K, H, W).  All float32, one rounding per operation, in this order:
 *   cx = 0.5f W, cy = 0.5f H, lerp(a, b, t) = fmaf(t, b - a, a);  for s = 0 .. S-1:
 *     us = fmaf(x - cx, inv[s], cx), vs = fmaf(y - cy, inv[s], cy);  pass s counts iff 0 <= us <= W-1 and 0 <= vs <= H-1 (inclusive);
 *     x0 = floor(us), x1 = min(x0 + 1, W-1), lx = us - x0, same for y;
 *     f = 0, m = stack[(s*F)*B + b, k]:            acc += lerp(lerp(m[y0][x0], m[y0][x1], lx), lerp(m[y1][x0], m[y1][x1], lx), ly), n += 1
 *     f = 1, m = stack[(s*F+1)*B + b, partner[k]]: the same with columns W-1-x0 and W-1-x1 (same lx, no one-pixel shift),    n += 1
 *   out = acc / n, or 0 when no pass sees the pixel.
 * Passes that cannot see a pixel do not dilute it.  S = 1, inv = 1, F = 2 is bit for bit pk_flip_merge on finite maps.             */
int pk_multiscale_merge(const float* stack, const int32_t* partner, const float* inv_scales_host, float* out,
                        int S, int F, int B, int K, int H, int W, void* stream);

/* ---- video post-processing (utils/postprocess.py:187-267) -------------------------------------------------------
 * pk_temporal_smooth: coords/out (T, C=2K) fp32, weights: `window` doubles as np.convolve receives them (the kernel is flipped
 * like np.convolve does; edge padding window/2 on both sides; float64 accumulation, float32 result); window must be odd.
 * pk_nms_pose: greedy in-sample suppression, preds (B,K,2), maxvals (B,K), out (B,K,2) = preds * keep, keep (B,K) uint8.     */
int pk_temporal_smooth(const float* coords, float* out, const double* weights, int T, int C, int window, void* stream);
int pk_nms_pose(const float* preds, const float* maxvals, float* out, uint8_t* keep, int B, int K, float distance_threshold,
                void* stream);

/* ---- movement analysis and PCK on pose sequences (this project's own specification, DESIGN.md "Movement analysis and PCK": the reference
 * imports calculate_movement_amplitude / calculate_temporal_consistency from utils.metrics -- examples/quick_start.py:159,
 * visualization.py:385,441 -- and names PCK in both yamls, and defines none of them).  One launch each; no float atomics; every
 * floating-point sum in a fixed order, so two runs give identical bits.
 * pk_pck: pred, gt (N,K,2) f32; vis (N,K) f32; norm (N) f32; thresholds (n_thr) f32, 1 <= n_thr <= PK_PCK_MAX_THR.  correct (n_thr,K) int64, valid (K)
 *   int64 and err_sum (K) float64 ACCUMULATE: the caller zeroes them once, every launch adds its batch.  Pair (n,k) counts iff vis > 0,
 *   norm[n] > 0 and the four coordinates are finite.  Decision in float32, one rounding per operation, no square root:
 *   dx = px - gx, dy = py - gy, d2 = dx dx + dy dy, r = thr norm, hit iff d2 <= r r.  err_sum[k] += sum_n sqrt((double)d2) / (double)norm[n].
 * pk_motion_stats: coords (S,T,K,2) f32 image pixels; conf (S,T,K) f32 or NULL; stats (S,K,11) float64, every element written.  Frame t of
 *   joint k is valid iff both coordinates are finite and (conf == NULL or conf >= min_conf); a step t -> t+1 counts iff both frames are
 *   valid, a triple iff t-1, t, t+1 are.  Columns: 0 n_valid; 1-4 min_x, max_x, min_y, max_y of the valid frames (0 without one);
 *   5 amplitude = sqrt((max_x - min_x)^2 + (max_y - min_y)^2); 6 path length = sum over steps of |p[t+1] - p[t]|; 7 n_steps; 8 largest
 *   step; 9 sum over triples of |(p[t+1] - 2 p[t]) + p[t-1]|; 10 n_triples.  Differences, norms sqrt(dx dx + dy dy) and sums in float64.
 * pk_position_histogram: edges_x (nbx+1), edges_y (nby+1) float64 ascending, on the device; counts (S,K,nby,nbx) int32, overwritten.  A
 *   valid frame (as above) falls in bin i with e[i] <= v < e[i+1], the last bin also takes v == e[nb], anything outside [e[0], e[nb]] is
 *   dropped: np.histogram2d's rule for any edges.  nbx nby <= PK_HIST_MAX_BINS (one workgroup's LDS histogram), else PK_ERR_UNSUPPORTED.  */
#define PK_PCK_MAX_THR 16
#define PK_HIST_MAX_BINS 16384
int pk_pck(const float* pred, const float* gt, const float* vis, const float* norm, const float* thresholds, int64_t* correct,
           int64_t* valid, double* err_sum, int N, int K, int n_thr, void* stream);
int pk_motion_stats(const float* coords, const float* conf, double* stats, int S, int T, int K, float min_conf, void* stream);
int pk_position_histogram(const float* coords, const float* conf, const double* edges_x, const double* edges_y, int32_t* counts,
                          int S, int T, int K, int nbx, int nby, float min_conf, void* stream);

/* ---- movement frequency spectrum of pose sequences (this project's own specification: DESIGN.md "Movement spectrum") -----------------
 * pk_motion_spectrum: coords (S,T,K,2) f32 image pixels; conf (S,T,K) f32 or NULL; frames are valid as for pk_motion_stats.  power (S,K,F)
 *   and summary (S,K,6) float64, every element written.  Two launches; no float atomics, every sum in a fixed order that depends on T
 *   alone: two launches give identical bits, and a bin's bits depend neither on S, on K nor on the other bins of the launch.
 *   Bin j (0 <= j < F) is the frequency (j0 + j) / N cycles per frame; j0 >= 1, j0 + F - 1 <= N / 2, 2 <= N <= PK_SPEC_MAX_NFFT = 2^30 (N > T zero-pads),
 *   1 <= F <= PK_SPEC_MAX_BINS.  window 0: w_t = 1; window 1: periodic Hann, w_t = 0.5 - 0.5 cos(6.283185307179586 ((double)t / (double)T)); an invalid
 *   frame has weight 0.  Per joint, in float64 without FMA: n = valid frames, W = sum w_t, m = sum w_t p_t / W, u_t = w_t (p_t - m),
 *   X_j = sum_t u_t.x (cos ang, sin ang) and Y_j likewise with r = ((int64)(j0 + j) t) mod N, ang = 6.283185307179586 ((double)r / (double)N),
 *   P_j = (4 / (W W)) ((Xre^2 + Xim^2) + (Yre^2 + Yim^2)): a linear oscillation of amplitude A px at a bin frequency has P = A^2.  n < 2 or
 *   not W > 0: the whole row is 0.  Summary columns: 0 n; 1 W; 2 band power sum_j P_j; 3 peak bin j0 + argmax_j P_j (the lowest among equal
 *   maxima; -1 when column 2 is 0); 4 the peak's power (or 0); 5 centroid sum (j0 + j) P_j / sum P_j in bins (or 0).                      */
#define PK_SPEC_MAX_BINS 16384
#define PK_SPEC_MAX_NFFT 1073741824
int pk_motion_spectrum(const float* coords, const float* conf, double* power, double* summary, int S, int T, int K, float min_conf,
                       int N, int j0, int F, int window, void* stream);

/* ---- limb kinematics of pose sequences (this project's own specification: DESIGN.md "Limb kinematics") ------------------------------
 * coords (S,T,K,2) f32 image pixels, conf (S,T,K) f32 or NULL, frames valid as for pk_motion_stats.  A SERIES is a float64 array (S,T,Q) whose
 * element is valid iff it is finite: the first two entries write NaN for "no value".  No float atomics, no global atomics; float64 on
 * exactly widened inputs, one rounding per operation, every floating-point sum in the fixed order of pk_motion_stats: two launches give
 * identical bits.
 * pk_joint_angles: triples (A,3) int32 on the device, joints (a, b, c) in [0, K) with a != b and b != c, 1 <= A <= PK_KIN_MAX_ANGLES; angles
 *   (S,T,A), every element written.  u = p_a - p_b, v = p_c - p_b, cr = u.x v.y - u.y v.x, dt = u.x v.x + u.y v.y, theta = atan2(|cr|, dt) in
 *   [0, pi]: the unsigned interior angle at b.  NaN when one of the three joints is invalid or a ray has no length (not u.u > 0 or not
 *   v.v > 0), and for a triple that breaks the rule above (the caller checks its host copy; the kernel never reads out of range).
 * pk_joint_speeds: speeds (S,T,K): sqrt(dx dx + dy dy) of p[t+1] - p[t] when frames t and t + 1 are valid, else NaN; the last frame is NaN.
 * pk_series_stats: stats (S,Q,PK_KIN_STATS_COLS).  Columns: 0 n valid; 1 minimum, 2 maximum (0 without a valid element); 3 mean = sum x / n
 *   (0 when n = 0); 4 population sd = sqrt(sum (x - mean)^2 / n) with the mean as stored in column 3 (0 when n = 0); 5 sum |x[t+1] - x[t]|
 *   over the steps whose two ends are valid; 6 the number of such steps; 7 the largest such step.
 * pk_series_xcorr: pairs (P,2) int32 on the device, series (i, j) in [0, Q); 0 <= max_lag = L <= PK_KIN_MAX_LAG; min_count >= 2.  corr (S,P,2L+1)
 *   float64 and count (S,P,2L+1) int32: lag index l' is the lag l = l' - L; over V = {t : 0 <= t, t + l < T, x_i[t] and x_j[t + l] valid},
 *   n = |V|: mx = sum x / n, my = sum y / n, sxx = sum (x - mx)^2, syy = sum (y - my)^2, sxy = sum (x - mx)(y - my), r = sxy / sqrt(sxx syy);
 *   r = 0 when n < 2 or not sxx syy > 0.  The pairs of a lag are summed in the order of the EARLIER of their two frames, so a lag's bits
 *   depend on T and the two series alone (not on S, P, L or the other lags) and (i, j) at l equals (j, i) at -l bit for bit.  summary (S,P,4)
 *   from the stored r and counts over the lags with count >= min_count: 0 r at lag 0 (0 if that lag does not qualify); 1 the lag l of the
 *   largest r (the lowest l' among equal maxima); 2 that r; 3 that lag's count; 1-3 are 0 without a qualifying lag.  Two launches.
 * pk_sample_entropy: tol (S,Q) float64, the absolute tolerance of each series; 1 <= m <= PK_KIN_MAX_M; T <= PK_KIN_MAX_T, else
 *   PK_ERR_UNSUPPORTED.  counts (S,Q,3) int64: 0 |W|, W = {i : 0 <= i <= T - m - 1, x[i .. i + m] all valid}; 1 B and 2 A, the pairs i < j of W
 *   with max_{k<m} |x[i+k] - x[j+k]| <= tol and max_{k<=m} ... <= tol: fabs(a - b) <= tol in float64, equality is a match.  A tolerance that
 *   is not finite or is negative gives (|W|, 0, 0).  SampEn = -ln(A / B) is the caller's.  workspace: S Q pk_sample_entropy_tiles(T, m) rows of
 *   2 int64 (never NULL: one row for a query of 0), every row written: the template starts are cut into blocks of PK_KIN_ENTROPY_TILE and one
 *   workgroup counts one pair of blocks; a second launch adds the rows.  pk_sample_entropy_tiles: nb (nb + 1) / 2 with
 *   nb = ceil((T - m) / PK_KIN_ENTROPY_TILE); 0 for T <= m, T > PK_KIN_MAX_T or an m out of range.                                       */
#define PK_KIN_MAX_ANGLES 64
#define PK_KIN_MAX_LAG 4096
#define PK_KIN_MAX_M 4
#define PK_KIN_MAX_T 262144
#define PK_KIN_STATS_COLS 8
#define PK_KIN_ENTROPY_TILE 256
int pk_joint_angles(const float* coords, const float* conf, const int32_t* triples, double* angles, int S, int T, int K, int A,
                    float min_conf, void* stream);
int pk_joint_speeds(const float* coords, const float* conf, double* speeds, int S, int T, int K, float min_conf, void* stream);
int pk_series_stats(const double* series, double* stats, int S, int T, int Q, void* stream);
int pk_series_xcorr(const double* series, const int32_t* pairs, double* corr, int32_t* count, double* summary, int S, int T, int Q, int P,
                    int max_lag, int min_count, void* stream);
int pk_sample_entropy_tiles(int T, int m);
int pk_sample_entropy(const double* series, const double* tol, int64_t* workspace, int64_t* counts, int S, int T, int Q, int m,
                      void* stream);

/* ---- localisation error analysis (this project's own specification, DESIGN.md "Localisation error analysis": the numbers behind the
 * reference's PerformanceAnalyzer, analysis/nn_quantitative_viz.py:105-252).  One launch each; no float atomics, no global atomics; every
 * output is an integer count, an order statistic or a fixed-order sum, so the same input gives the same bits.
 * pk_kpt_error: pred, gt (N,K,2) f32; vis (N,K) f32; conf (N,K) f32 or NULL; norm (N) f32 or NULL.  err_out is a (K, ld) f32 matrix, ld >= N:
 *   this launch writes columns 0..N-1 of each row (the caller passes the pointer already offset to its first free column).  calib_count,
 *   calib_hit (K, n_bins) int64 and pr_hist (K, 2, T+1) int64 ACCUMULATE: the caller zeroes them once, every launch adds its batch.
 *   Pair (n,k) counts iff vis > 0, its four coordinates are finite and, when norm is given, norm[n] > 0 (pk_pck's rule); an uncounted pair
 *   writes NaN to err_out and touches no counter.  Error in float32, one rounding per operation, no FMA: dx = px - gx, dy = py - gy,
 *   d2 = dx dx + dy dy, e = (float)sqrt((double)d2); with norm e = (float)((double)e / (double)norm[n]).  Both narrowings equal the correctly
 *   rounded float32 operation and do not depend on how sqrtf or / are lowered.  hit = e < pixel_thr (strict).
 *   conf == NULL: bin_edges, conf_thr and the three counters may be NULL as well; only the store is written.  With conf: a pair whose
 *   confidence c is not finite stays in the store and enters neither calibration nor precision / recall.  Calibration: bin i of the
 *   ascending bin_edges (n_bins + 1) takes e[i] <= c < e[i+1], anything outside is dropped, c == e[n_bins] included (the reference's rule,
 *   not np.histogram's); there calib_count += 1, calib_hit += hit.  Precision / recall: m = the number of the ascending conf_thr (T) with
 *   c > t_i, 0 <= m <= T; pr_hist[k][hit ? 0 : 1][m] += 1.  The host recovers the reference's counts at threshold i by suffix sums:
 *   tp_i = sum_{m>i} pr_hist[.,0,m], fp_i = sum_{m>i} pr_hist[.,1,m], fn_i = sum_m pr_hist[.,0,m] - tp_i.
 *   Refused before the launch: a null required pointer, N or K <= 0, ld < N, and with conf n_bins outside 1..PK_ERR_MAX_BINS or T outside
 *   1..PK_ERR_MAX_CONF_THR (the int32 histograms one workgroup keeps in LDS).
 * pk_kpt_error_quantiles: err (K, ld) f32, columns 0..n_cols-1 of each row; a NaN entry does not exist, every other value is non-negative
 *   (its unsigned bit pattern orders it).  q (Q) float64 on the device, each in [0,1].  Per row with n values v[0] <= ... <= v[n-1]:
 *   pos = q (double)(n - 1), lo = floor(pos), hi = min(lo + 1, n - 1); order (K,Q,2) f32 = v[lo], v[hi], found exactly by radix select over the
 *   float bits (the interpolation between the two is the host's).  summary (K,4) float64 = n, sum, min, max; the sum in float64, per
 *   thread in ascending column, then the block reduction.  n = 0: every output of the row is 0.
 *   Refused before the launch: a null pointer, Q outside 1..PK_ERR_MAX_QUANTILES, K <= 0, n_cols outside 1..PK_ERR_MAX_COLS = 2^31 - 1, ld < n_cols.        */
#define PK_ERR_MAX_BINS 256
#define PK_ERR_MAX_CONF_THR 1024
#define PK_ERR_MAX_QUANTILES 16
#define PK_ERR_MAX_COLS 2147483647
int pk_kpt_error(const float* pred, const float* gt, const float* vis, const float* conf /* or NULL */, const float* norm /* (N) or NULL */,
                 float pixel_thr, const float* bin_edges /* (n_bins+1) */, int n_bins, const float* conf_thr /* (T) ascending */, int T,
                 float* err_out, int64_t ld, int64_t* calib_count, int64_t* calib_hit, int64_t* pr_hist, int N, int K, void* stream);
int pk_kpt_error_quantiles(const float* err, int64_t ld, int64_t n_cols, int K, const double* q /* (Q) device, each in [0,1] */, int Q,
                           float* order /* (K,Q,2) */, double* summary /* (K,4) */, void* stream);

/* ---- occlusion sensitivity (this project's own specification, DESIGN.md "Occlusion sensitivity": the map of the reference's
 * SensitivityAnalyzer.occlusion_sensitivity, analysis/advanced_analysis.py:387-427, for every joint from one batched sweep).  No atomics;
 * the one floating-point sum is taken in a fixed order, so the same input gives the same bits.
 * Grid: patch rows start at range(0, H - patch, stride), columns likewise: per axis n(extent) = ceil((extent - patch) / stride) positions
 *   when extent > patch, else none; the position extent - patch itself is NOT taken (the reference's rule, kept).  ny = n(H), nx = n(W);
 *   copy p = a nx + b blanks rows a stride .. a stride + patch - 1 and columns b stride .. b stride + patch - 1.  An empty grid is
 *   PK_ERR_INVALID in every entry below.
 * pk_occlusion_positions: host only, returns n(extent) >= 0; PK_ERR_INVALID (with the error text set) for extent, patch or stride < 1.
 * pk_occlude_batch: x (H,W,8) bf16, the stem's packed image; out (n,H,W,8) bf16 receives copies first .. first + n - 1: the image with
 *   the patch's pixels replaced by the fill.  fill_host: HOST pointer to 3 floats (read before the call returns, rounded to bf16 to nearest
 *   even as pk_nchw_f32_to_nhwc_bf16 rounds, carried in the kernel's arguments) or NULL = 0, the mean in normalised space; channels 3..7
 *   of a filled pixel are 0.  One 16-byte load and one 16-byte store per pixel.  Refused before the launch: a null or misaligned pointer,
 *   first < 0, n < 1, first + n > ny nx, n H W >= 2^32 - 1, and a source that overlaps the destination.
 * pk_heatmap_summary: heatmaps (M,h,w) fp32; out (M,4) float64 = sum, max, argmax x, argmax y.  One 256-thread workgroup per map
 *   (workgroups stride over the maps when M exceeds the grid).  Sum: thread t adds elements t, t + 256, ... in ascending order to 0.0 in
 *   float64; then the xor butterfly 32, 16, ..., 1 inside each wave, then wave 0 + wave 1 + wave 2 + wave 3.  Maximum: a candidate is
 *   replaced iff v > best in float32, starting from -inf without an index; among equal values (-0 = +0) the smallest flat index wins; a
 *   NaN never wins and makes the sum NaN; a map with no value above -inf reports max = -inf at index 0.  max is the element at the winning
 *   index, widened; x = idx % w, y = idx / w, exact.
 * pk_occlusion_paint: base (K,4) and table (P = ny nx, K, 4) rows of pk_heatmap_summary; maps (K,H,W) float64, every element written once.
 *   The reference writes map[i : i + patch, j : j + patch] = base - score in loop order, the last writer wins; in closed form pixel (y, x)
 *   has a = min(y / stride, ny - 1), b = min(x / stride, nx - 1), is covered iff y < a stride + patch and x < b stride + patch, and then takes
 *   the value of copy a nx + b; an uncovered pixel is 0.  measure 0: base.sum - t.sum; 1: base.max - t.max; 2: sqrt(dx dx + dy dy) of the
 *   two argmax positions, in float64 without FMA.                                                                                   */
int pk_occlusion_positions(int extent, int patch, int stride);
int pk_occlude_batch(const void* x /* (H,W,8) bf16 */, void* out /* (n,H,W,8) bf16 */, int H, int W, int patch, int stride, int first, int n,
                     const float* fill_host /* 3 floats or NULL */, void* stream);
int pk_heatmap_summary(const float* heatmaps /* (M,h,w) */, double* out /* (M,4): sum, max, argmax x, argmax y */, int64_t M, int h, int w,
                       void* stream);
int pk_occlusion_paint(const double* base /* (K,4) */, const double* table /* (P,K,4) */, double* maps /* (K,H,W) */, int measure, int K,
                       int H, int W, int patch, int stride, void* stream);

/* ---- L1/L2: FusionPoseLoss.forward (models/fusion_head.py:745-806 with :405-559, :637-743) ---------------
 * stats: workspace of B*K*PK_LOSS_STAT floats + B*16*4 floats + 16 floats (see PK_LOSS_WS_FLOATS);
 * losses: 7 floats (heatmap, offset, peak, variance, overlap, shape, total — already multiplied by lambdas).
 * lambdas7: device array of 7 floats = the six term weights + the overlap threshold (GaussianDistributionConstraint, default 0.5). */
#define PK_LOSS_STAT 24
#define PK_LOSS_WS_FLOATS(B, K) ((B) * (K) * PK_LOSS_STAT + (B) * 16 * 4 + 16)
int pk_fusion_loss_fwd(const float* heatmaps, const float* offsets, const float* variances, const float* target,
                       const float* weight, const float* gt_keypoints, float* ws, float* losses,
                       int B, int K, int H, int W, float in_w, float in_h, float sigma_t,
                       const float* lambdas7, int use_target_weight /* 0: heatmap/offset/peak terms are plain (B,K) means */, void* stream);
int pk_fusion_loss_bwd(const float* heatmaps, const float* offsets, const float* variances, const float* target,
                       const float* weight, const float* ws, const float* grad_total /*device scalar or NULL=1*/,
                       float* d_heatmaps, float* d_offsets, float* d_variances,
                       int B, int K, int H, int W, float sigma_t, const float* lambdas7, void* stream);

/* The same terms with COORDINATES HANDED IN by the caller: the public methods GaussianDistributionConstraint.compute_heatmap_variance /
 * variance_alignment_loss / spatial_overlap_loss / distribution_shape_loss / forward (models/fusion_head.py:405-575) and
 * FusionPoseLoss.heatmap_loss / offset_loss / peak_localization_loss (:637-743) take any (B,K,2) coordinates, not only the map's own
 * soft-argmax.  coords == NULL is pk_fusion_loss_fwd.  sigma (B,K) or NULL receives compute_heatmap_variance's result.  Backward:
 * d_coords (B,K,2) receives the coordinate gradient (NULL: the coordinates were the soft-argmax, their gradient flows into d_heatmaps);
 * grad_sigma (B,K) or NULL is an upstream gradient on `sigma`.  A term is selected by its lambda (0 elsewhere).                         */
int pk_fusion_terms_fwd(const float* heatmaps, const float* offsets, const float* variances, const float* target,
                        const float* weight, const float* gt_keypoints, const float* coords, float* ws, float* losses, float* sigma,
                        int B, int K, int H, int W, float in_w, float in_h, float sigma_t,
                        const float* lambdas7, int use_target_weight, void* stream);
int pk_fusion_terms_bwd(const float* heatmaps, const float* target, const float* ws, const float* grad_total,
                        const float* grad_sigma, const float* grad_losses /* 7 upstream gradients of `losses` or NULL (= total only) */,
                        float* d_heatmaps, float* d_offsets, float* d_variances, float* d_coords,
                        int B, int K, int H, int W, float sigma_t, const float* lambdas7, void* stream);
/* LocalGaussianRefinement.forward (models/fusion_head.py:74-128) about given coordinates; backward of SoftArgmax2D.forward (:24-71)        */
int pk_local_gaussian_refine(const float* heatmaps, const float* coords_in, float* coords_out, int BK, int H, int W,
                             int local_radius, void* stream);
int pk_softargmax_bwd(const float* heatmaps, const float* coords, const float* scores, const float* grad_coords,
                      const float* grad_scores, float* d_heatmaps, int BK, int H, int W, void* stream);

/* ---- L3/L4: KeypointMSELoss (models/pose_estimator.py:102-143) and models/losses.py per-pixel losses ------
 * kind 0: mean(((p-t)*w)^2)  [KeypointMSELoss]; 1: mean(w*(p-t)^2) [FusedPoseLoss mse];
 * 2: mean(w*smoothl1(p-t)) [FusedPoseLoss smoothl1]; 3: JointsMSELoss (0.5*mean((p-t)^2 w^2)).
 * partial: workspace of PK_REDUCE_BLOCKS floats.                                                            */
#define PK_REDUCE_BLOCKS 1024
int pk_pixel_loss_fwd(const float* pred, const float* target, const float* weight, float* partial, float* loss,
                      int B, int K, int HW, int kind, void* stream);
int pk_pixel_loss_bwd(const float* pred, const float* target, const float* weight, const float* grad_out,
                      float* d_pred, int B, int K, int HW, int kind, void* stream);
/* Online hard keypoint mining (CPN; HRNet's JointsOHKMMSELoss, mmpose's KeypointOHKMMSELoss): per sample only the `topk` maps with the
 * largest error count.  L[b,k] = (1/HW) sum_i (w[b,k] (pred - target))^2;  selected: the topk largest L of the sample in torch.topk's
 * order (descending, a NaN before every number, equal values and NaNs among themselves by lower joint index);
 * mask[b,k] = 1 for the selected maps;  loss = scale / (B topk) * sum of the selected L;  counts[k] += sum_b mask[b,k] (counts may be NULL).
 * d_pred = mask * G * scale * 2 w^2 (pred - target) / (HW topk B), zero (and stored) for unselected maps; nothing flows through the
 * selection.  weight (B,K) or NULL = 1; a map with w = 0 has L = 0, may be selected when fewer than topk are non-zero, and adds nothing.
 * topk = K is the plain weighted mean (pixel loss kind 0 times scale).  Refused before any launch: a null required pointer, B or HW <= 0,
 * K outside 1..PK_OHKM_MAX_K, topk outside 1..K, a scale that is not finite and positive.  Three launches in all (per-map sums, a
 * one-workgroup selection, the gradient), no atomics, no host synchronisation: the same input gives the same bits.               */
#define PK_OHKM_MAX_K 256
int pk_ohkm_loss_fwd(const float* pred, const float* target, const float* weight /* (B,K) or NULL = 1 */,
                     float* per_map /* (B,K) out */, uint8_t* mask /* (B,K) out */, float* loss /* 1 out */,
                     int64_t* counts /* (K) in/out, or NULL */, int B, int K, int HW, int topk, float scale, void* stream);
int pk_ohkm_loss_bwd(const float* pred, const float* target, const float* weight, const uint8_t* mask,
                     const float* grad_out /* 1, or NULL = 1 */, float* d_pred, int B, int K, int HW, int topk, float scale, void* stream);
/* MorphologyShapeLoss statistics (models/losses.py:69-104): mean (BK,2), variance (BK,2) of hm/(sum+1e-8) */
int pk_spatial_stats(const float* heatmaps, float* mean, float* var, int BK, int H, int W, void* stream);
/* backward of pk_spatial_stats (MorphologyShapeLoss, models/losses.py:50-135): grad_mean / grad_var (BK,2) -> grad_heatmaps */
int pk_spatial_stats_bwd(const float* heatmaps, const float* mean, const float* var, const float* grad_mean, const float* grad_var,
                         float* grad_heatmaps, int BK, int H, int W, void* stream);

/* ---- S1: AdamW on one flat fp32 buffer (train.py:55-97 grouping; torch.optim.AdamW arithmetic) -----------
 * decay_mask: 1 byte per element (1 = apply weight decay).  lr/step come from DEVICE scalars so a captured
 * graph can be replayed while the schedule advances.  Also refreshes the bf16 compute copy (may be NULL).   */
int pk_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                  uint16_t* param_bf16, int64_t n, const float* lr_dev, const int32_t* step_dev,
                  float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream);
/* Guarded step (opt-in; what GradScaler.step + clip_grad_norm_ do around optimizer.step in the reference's train.py:182-184): three
 * launches on one stream, no atomics, no host read, every sum in a fixed order.
 * pk_grad_sumsq: fp64 sum of grad^2 over the elements whose flag has bit1 set (the ones pk_adamw_step updates; everything else is
 *   ignored whatever it holds).  partials: 2 doubles per workgroup {sum, 1.0 if an element had all exponent bits set else 0.0};
 *   n_partials must be pk_grad_sumsq_partials(n), the grid size (a function of n only).
 * pk_grad_guard_finalize: norm = grad_scale*sqrt(total); c = max_norm/(norm+1e-6); coef = (max_norm>0 && finite && c<1) ? c : 1
 *   (torch.nn.utils.clip_grad_norm_); skip = any non-finite flag.  guard_state: 4 words {float norm, float coef, int32 skipped_last,
 *   int32 skipped_total (+1 on skip)}.  step_dev[0] += 1 only when the step is NOT skipped (it counts applied updates).
 * pk_adamw_step_guarded: pk_adamw_step with gradient factor grad_scale*coef; touches nothing when skipped_last is set.  With
 *   coef == 1 the result is bitwise pk_adamw_step's.                                                                            */
int pk_grad_sumsq_partials(int64_t n);
int pk_grad_sumsq(const float* grad, const uint8_t* flags, int64_t n, double* partials, int n_partials, void* stream);
int pk_grad_guard_finalize(const double* partials, int n_partials, float grad_scale, float max_norm, int32_t* guard_state,
                           int32_t* step_dev, void* stream);
int pk_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                          uint16_t* param_bf16, int64_t n, const float* lr_dev, const int32_t* step_dev,
                          float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                          const int32_t* guard_state, void* stream);
/* Weight EMA (opt-in): the update of pk_adamw_step (guard_state NULL) or of pk_adamw_step_guarded (guard_state given), and in the same
 * pass, for every element whose flag has bit1 set, ema += (1 - d_t) * (param_new - ema) in fp32 with param_new taken from registers.
 * d_t = min(ema_decay, (1 + t) / (10 + t)) with t = (float)step_dev[0], the bias correction's t (applied updates, >= 1), computed on
 * the device in every launch: a replayed graph and a guarded run advance the warm-up without a host write.  Elements without bit1
 * keep their ema bits.  A skipped step (guard_state[2] set) touches nothing, ema included.  param, exp_avg, exp_avg_sq and the bf16
 * copy come out bitwise as from the entry point it stands in for.  ema: n floats, 16-byte aligned, not overlapping param;
 * 0 < ema_decay < 1.  36 bytes per element instead of 28.                                                                        */
int pk_adamw_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                      uint16_t* param_bf16, int64_t n, const float* lr_dev, const int32_t* step_dev,
                      float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                      const int32_t* guard_state, float* ema, float ema_decay, void* stream);
/* Per-tensor statistics of a flat fp32 buffer (opt-in diagnostics: which tensor was non-finite, gradient flow, weight scale, update
 * size): a segmented reduction in two launches, no atomics, every sum in an order the plan fixes (same bits eager, on any stream, replayed).
 * x = a[i], or with b given a[i] - b[i] rounded once to fp32; an element takes part iff flags == NULL or its flag has bit1 set.
 * Segment table (host): n_tensors rows {int64 offset, int64 count}; offsets in elements and multiples of 4, counts >= 1.  Elements between
 * offset + count and the next offset are padding and are never read.
 * Record (PK_TENSOR_STATS_RECORD_BYTES each, table order):
 *   +0 f64 sum x | +8 f64 sum x^2 (squares formed in fp64) | +16 f64 sum |x| | +24 f32 min (+inf if none) | +28 f32 max (-inf if none)
 *   | +32 i64 participating elements | +40 i64 of them inf / NaN (exponent bits all ones) | +48 i64 finite with |x| <= tiny | +56 i64 0.
 *   Sums, min, max and the small count run over the finite participating elements only.
 * pk_tensor_stats_plan: builds the launch plan on the host from the table and returns the item count (one item per tensor and chunk of
 *   pk_tensor_stats_chunk_elems() elements); plan_out_host NULL: count only.  The plan is pk_tensor_stats_plan_bytes(n_items, n_tensors)
 *   bytes: 16-byte rows, n_tensors of {int32 first_item, int32 n_items, int64 0}, then n_items of {int64 first element, int32 count,
 *   int32 tensor}; it carries the table, so the device needs no other copy of it.  The caller uploads it once.
 * pk_tensor_stats: partial kernel (one wave per item, four items per workgroup) and finalize kernel (one wave per tensor).  ws:
 *   pk_tensor_stats_ws_bytes(n_items, n_tensors) bytes; a, b, plan, ws, records 16-byte aligned, flags 4-byte; tiny finite and >= 0.
 *   The caller guarantees that a, b and flags cover every offset + count of the table.
 * pk_tensor_stats_latch: one workgroup.  If any record has a non-finite count > 0: latched <- all n_tensors records, latch_state
 *   (4 int32) = {events + 1, first offending tensor, last offending tensor, offending tensors}.  Otherwise nothing is written.        */
#define PK_TENSOR_STATS_RECORD_BYTES 64
int pk_tensor_stats_chunk_elems(void);
int pk_tensor_stats_plan(const int64_t* seg_host, int n_tensors, void* plan_out_host, int64_t capacity_bytes);
int pk_tensor_stats_plan_bytes(int n_items, int n_tensors);
int pk_tensor_stats_ws_bytes(int n_items, int n_tensors);
int pk_tensor_stats(const float* a, const float* b, const uint8_t* flags, const void* plan_dev, int n_tensors, int n_items, float tiny,
                    void* ws, int64_t ws_bytes, void* records, void* stream);
int pk_tensor_stats_latch(const void* records, int n_tensors, void* latched, int32_t* latch_state, void* stream);

/* ---- activation statistics (this project's own specification, DESIGN.md "Activation statistics": the numbers behind the reference's
 * ActivationAnalyzer, analysis/advanced_analysis.py:34-125, without its copy of every feature map to the host).  x: bf16, M rows x C
 * channels, row-major (an NHWC map flattened), 16-byte aligned; C % 8 == 0, 8 <= C <= PK_ACT_MAX_CHANNELS, 1 <= M C <= PK_ACT_MAX_ELEMS
 * = 2^38; 1 <= c_used <= C: channels >= c_used are padding and take part in nothing.  No global atomics, no float atomics, no last-arriver:
 * the same input gives the same bits on any stream.
 * Element rule: exponent bits all ones (inf / NaN) -> counted in n_nonfinite and left out of everything else (pk_tensor_stats' rule).
 * Record (PK_ACT_RECORD_BYTES each, one per channel < c_used):
 *   +0 f64 sum x | +8 f64 sum x^2 (squares formed in fp64) | +16 f32 min (+inf if none) | +20 f32 max (-inf if none) | +24 i64 n (all
 *   elements of the channel, M per call) | +32 i64 +-0 | +40 i64 x < 0 | +48 i64 inf / NaN | +56 i64 0.  min / max read -0 as +0.
 * Table: PK_ACT_HIST_BINS int64 counts over the finite elements of the channels < c_used.  key = the bf16 bits made sortable (-0 first
 *   mapped to +0; sign set -> ~bits, else bits | 0x8000), bin = key >> 4: sign, exponent and three mantissa bits, so the edges are exact
 *   bf16 values and the same for every tensor; +0 lies in bin 2048.
 * Split: CH = C / 8 threads cover a row, G = 256 / CH rows are read per pass of a 256-thread workgroup, a slab is
 *   pk_activation_stats_slab(C) = 4 G rows, B = pk_activation_stats_blocks(M, C) = min(512, ceil(M / slab)) workgroups, workgroup b takes
 *   slabs b, b + B, ...  Order of the two sums, per channel: thread (b, r) adds its rows s slab + u G + r in ascending (s, u) to 0.0; the
 *   workgroup adds its threads r = 0, 1, ..., G - 1 from left to right; the finalize adds the workgroups g, g + 16, g + 32, ... in ascending
 *   order to 0.0 in each of 16 groups g, then the groups 0, 1, ..., 15 from left to right.
 *   +-0 are counted in registers and enter the table in the finalize, never as LDS atomics.
 * pk_activation_stats: two launches.  ws: pk_activation_stats_ws_bytes(M, C) bytes, 16-byte aligned, as x and records; hist 8-byte.
 *   accumulate != 0: every field of the records and the table becomes old + new (new computed as above), min / max are combined;
 *   accumulate == 0 overwrites.
 * pk_activation_quantiles: exact order statistics of the finite elements of the channels < c_used, three launches.  hist: the table of
 *   pk_activation_stats of the same x and c_used.  q_host: HOST pointer to Q <= PK_ACT_MAX_QUANTILES doubles in [0, 1], read before the
 *   call returns.  With the n finite values v[0] <= ... <= v[n-1] (-0 == +0): pos = q (double)(n - 1), lo = floor(pos), hi = min(lo + 1,
 *   n - 1) (pk_kpt_error_quantiles' rule); order (Q,2) f32 on the device = v[lo], v[hi]; a zero comes out as +0; n == 0: NaN.  A rank's bin
 *   is found in the table, one more pass over x counts the low four key bits inside the selected bins: bin and sub-bin are all 16 bits.
 *   ws: pk_activation_quantiles_ws_bytes(M, C) bytes, 16-byte aligned.
 * Refused before any launch, in this order: a null pointer; C % 8; C outside its range; c_used outside [1, C]; M C outside [1, 2^38]; Q;
 *   a q outside [0, 1] or NaN; misalignment; a workspace that is too small.  For a refused shape pk_activation_stats_blocks returns 0 (a count), the other queries PK_ERR_INVALID.      */
#define PK_ACT_RECORD_BYTES 64
#define PK_ACT_HIST_BINS 4096
#define PK_ACT_MAX_CHANNELS 2048
#define PK_ACT_MAX_QUANTILES 16
#define PK_ACT_MAX_ELEMS 274877906944
int pk_activation_stats_slab(int C);
int pk_activation_stats_blocks(int64_t M, int C);
int pk_activation_stats_ws_bytes(int64_t M, int C);
int pk_activation_stats(const void* x, int64_t M, int C, int c_used, void* ws, int64_t ws_bytes, void* records, int64_t* hist,
                        int accumulate, void* stream);
int pk_activation_quantiles_ws_bytes(int64_t M, int C);
int pk_activation_quantiles(const void* x, int64_t M, int C, int c_used, const int64_t* hist, const double* q_host, int Q, void* ws,
                            int64_t ws_bytes, float* order, void* stream);

/* ---- stochastic-depth ensembles (this project's own specification, DESIGN.md "Predictive uncertainty"): what S stacked outputs of one
 * input say together.  No atomics; every floating-point sum is taken in a fixed order, so the same input gives the same bits.
 * pk_ensemble_moments: element i of member s is stack[s member_stride + i], i < L, member_stride >= L.  Per element, in float64 and
 *   without FMA: m = (((0.0 + v_0) + v_1) + ... + v_{S-1}) / S; q = (((0.0 + (v_0 - m)^2) + (v_1 - m)^2) + ...), ascending s;
 *   mean[i] = m and std[i] = sqrt(q / (S - ddof)), each narrowed to fp32 round to nearest even.  NaN and inf propagate (an inf member gives
 *   mean inf and std NaN).  ddof 0 (np.std) or 1.  One thread per 16-byte group of four elements when L and member_stride are multiples of
 *   4 and the three pointers are 16-byte aligned, else one thread per element; a grid-stride loop over at most PK_ENS_GRID_CAP workgroups
 *   of 256.  S <= PK_ENS_REG_MEMBERS: the stack is read once, the members held in registers; above: two reads, sum then squares.  Both
 *   forms are the arithmetic above, bit for bit.  Refused before the launch: a null pointer; S < 1 + ddof; ddof outside 0..1; L < 1;
 *   member_stride < L; an output that overlaps the stack or the other output.
 * pk_ensemble_points: coords (S,M,2) fp32, conf (S,M) fp32 or NULL, centre (M,2) float64 or NULL, out (M,12) float64.  One 256-thread
 *   workgroup per point m (workgroups stride over m beyond PK_ENS_POINT_GRID_CAP).  Member s is valid iff both coordinates are finite and
 *   (conf == NULL or conf is finite and >= min_conf).  Every reduction is pk_heatmap_summary's: thread t takes the valid members among
 *   t, t + 256, ... in ascending order, starting from 0.0 (+inf for the minimum), then the xor butterfly 32, 16, ..., 1 inside each wave,
 *   then wave 0 op wave 1 op wave 2 op wave 3.  All arithmetic float64 without FMA.  First pass: n, sum x, sum y, sum conf, min conf;
 *   mx = sum x / n, my = sum y / n, mc = sum conf / n.  (cx, cy) = centre[m], or (mx, my) when centre == NULL.  Second pass, per valid
 *   member: dx = x - mx, dy = y - my, dc = conf - mc; the sums of dx dx, dy dy, dx dy, dc dc; and the count of members with
 *   (x - cx)(x - cx) + (y - cy)(y - cy) <= radius radius.  Columns: 0 n; 1, 2 mx, my; 3, 4, 5 vx, vy, c = those sums / (n - ddof);
 *   6, 7 the eigenvalues of [[vx, c], [c, vy]] (squared semi-axes of the 1-sigma ellipse): h = (vx + vy) 0.5, d = (vx - vy) 0.5,
 *   r = sqrt(d d + c c), l1 = h + r, l2 = h - r if that is > 0, else 0; 8, 9, 10 mc, sqrt(sum dc dc / (n - ddof)), min conf (all three 0
 *   when conf == NULL); 11 the agreement count.  n < 1 + ddof: the whole row is 0.  Refused before the launch: a null coords or out;
 *   S < 1 or M < 1; S M >= 2^61; a radius that is negative or not finite; ddof outside 0..1.                                        */
#define PK_ENS_REG_MEMBERS 32
#define PK_ENS_GRID_CAP 4096
#define PK_ENS_POINT_GRID_CAP 65536
#define PK_ENS_POINT_COLS 12
int pk_ensemble_moments(const float* stack, int64_t member_stride, int S, int64_t L, int ddof, float* mean, float* std, void* stream);
int pk_ensemble_points(const float* coords /* (S,M,2) */, const float* conf /* (S,M) or NULL */, const double* centre /* (M,2) or NULL */,
                       double* out /* (M,12) */, int S, int64_t M, float min_conf, double radius, int ddof, void* stream);

/* ---- gradient attribution (this project's own specification, DESIGN.md "Gradient attribution": input saliency and Grad-CAM of every
 * joint from one batched backward; the reference's SensitivityAnalyzer.compute_input_sensitivity, analysis/advanced_analysis.py:317-342,
 * and GradCAMVisualizer.generate_cam, analysis/nn_quantitative_viz.py:358-415).  No atomics; every reduction runs in a fixed order
 * (per thread ascending, then the block reduction of pk_heatmap_summary), so the same input gives the same bits.
 * pk_stem_dgrad: data gradient of the stem's 3x3, stride-2, pad-1 convolution.  g (B,Ho,Wo,Cout) bf16; w the FORWARD pack [Cout][9][8]
 *   bf16 (mode 0 of pk_pack_weights); dx (B,Hs,Ws,8) bf16.  dx[b,y,x,c] = sum over the taps t = ky 3 + kx ascending with y + 1 - ky and
 *   x + 1 - kx even and oy = (y + 1 - ky) / 2 < Ho, ox likewise < Wo (1, 2 or 4 taps per pixel), inside a tap over n ascending, of
 *   g[b,oy,ox,n] w[n][t][c]: fp32 products (exact) and additions, one rounding to bf16 at the end; channels >= c_real are exactly 0.
 *   One thread per input pixel, the pack staged once per workgroup in LDS.  Refused before the launch: a null or misaligned pointer;
 *   Cout not a multiple of 8 or above PK_STEM_DGRAD_MAX_COUT; c_real outside 1..8; Ho != (Hs - 1) / 2 + 1 or Wo likewise;
 *   B Hs Ws >= 2^31.
 * pk_nhwc_bf16_to_nchw_f32: g (B,H,W,Cpad) bf16 -> out (B,C,H,W) fp32, C <= Cpad, Cpad a multiple of 8: out[b,c,y,x] = g[b,y,x,c]
 *   widened (exact).  The backward of pk_nchw_f32_to_nhwc_bf16.
 * pk_saliency_reduce: g (B,H,W,8) bf16 -> out (B,H,W) fp32 = max over c < c_real of |g_c| (exact; -0 gives +0).  A NaN in a real channel
 *   gives NaN, as torch.max does; channels >= c_real are not looked at.
 * pk_gradcam: A and G (B,h,w,C) bf16, C a multiple of 8, 1 <= c_used <= C (channels >= c_used are ignored).  Per sample b, in float64
 *   without FMA: weight[c] = S_c / (h w), S_c the sum of G[b,p,c] over the pixels p in the order of pk_heatmap_summary's sum;
 *   raw[p] = max(0, ((0.0 + weight[0] A[b,p,0]) + weight[1] A[b,p,1]) + ... over c < c_used), a NaN staying NaN; lo, hi = minimum and
 *   maximum of raw; cam[b,p] = (raw[p] - lo) / ((hi - lo) + 1e-8) rounded once to fp32; weights (B,c_used) = weight rounded to fp32;
 *   range (B,2) = lo, hi.  A NaN in any raw value makes lo, hi and the sample's whole map NaN.  Two launches: one workgroup per
 *   (sample, 8-channel chunk) for the weights, one workgroup per sample for the map.  ws: float64 workspace of pk_gradcam_ws_floats
 *   4-byte floats (per sample the weights of 8 ceil(c_used / 8) channels and the h w raw values; 0 for an empty problem).            */
#define PK_STEM_DGRAD_MAX_COUT 256
int pk_stem_dgrad(const void* g /* (B,Ho,Wo,Cout) bf16 */, const void* w /* [Cout][9][8] bf16 */, void* dx /* (B,Hs,Ws,8) bf16 */, int B, int Hs,
                  int Ws, int Ho, int Wo, int Cout, int c_real, void* stream);
int pk_nhwc_bf16_to_nchw_f32(const void* g /* (B,H,W,Cpad) bf16 */, float* out /* (B,C,H,W) */, int B, int C, int H, int W, int Cpad, void* stream);
int pk_saliency_reduce(const void* g /* (B,H,W,8) bf16 */, float* out /* (B,H,W) */, int B, int H, int W, int c_real, void* stream);
int pk_gradcam_ws_floats(int B, int h, int w, int c_used);
int pk_gradcam(const void* A, const void* G /* (B,h,w,C) bf16 */, double* ws, float* cam /* (B,h,w) */, float* weights /* (B,c_used) */,
               double* range /* (B,2): min, max of raw */, int B, int h, int w, int C, int c_used, void* stream);

/* ---- feature sheets and heat-map quality (this project's own specification, DESIGN.md "Feature sheets and heat-map quality": the sheet of
 * colour-mapped channel tiles and the target / prediction / difference panels of the reference's FeatureVisualizer,
 * analysis/nn_quantitative_viz.py:255-324, and a record of quality numbers per pair of maps).  No atomics, no last-arriver; every
 * floating-point sum in a fixed order and the colour index a fixed sequence of fp32 operations without FMA, each rounded once (the
 * division correctly rounded): the same input gives the same bits on any stream.
 * pk_gather_planes: x (B,H,W,C) bf16 NHWC, C a multiple of 8, 16-byte aligned; channels (n) int32 on the device, 1 <= n <= PK_PANEL_MAX_TILES;
 *   out (n,H,W) fp32, every element written.  Plane i = channel channels[i] of sample b, widened (exact).  A channel outside [0, c_used)
 *   gives a plane of quiet NaN (0x7fc00000) and is never turned into an address.  One thread per pixel and run of 8 list entries: it
 *   loads the pixel's 16-byte channel group once per run of entries that fall into the same group and keeps the wanted lanes.
 *   Refused before the launch, in this order: a null pointer; B, H, W or C < 1 or H W > PK_PANEL_MAX_PLANE; C not a multiple of 8; b outside
 *   0..B-1; n outside 1..PK_PANEL_MAX_TILES; c_used outside 1..C; x not 16-byte or channels / out not 4-byte aligned.
 * pk_plane_sheet_size: host only.  rows = ceil(T / cols); *SH = pad + rows (h zoom + pad), *SW = pad + cols (w zoom + pad).  Refused, in
 *   this order: a null pointer; T outside 1..PK_PANEL_MAX_TILES; h or w < 1 or h w > PK_PANEL_MAX_PLANE; cols outside 1..PK_PANEL_MAX_TILES; zoom
 *   outside 1..PK_PANEL_MAX_ZOOM; pad outside 0..PK_PANEL_MAX_PAD; SH or SW above PK_PANEL_MAX_SIDE (the drawing unit's limit).
 * pk_plane_sheet: a (Na,h,w) fp32; b (Nb,h,w) fp32 or NULL with Nb = 0; tiles (T,3) int32 on the device = {ia, ib, ramp}; luts (L,256,3)
 *   uint8; ranges (T,2) fp32 and sheet (SH,SW,3) uint8, every element and every byte written (the caller hands over uninitialised memory).
 *   Element e = (i, j) of tile t has v = a[ia][e] when ib < 0, else fabsf(a[ia][e] - b[ib][e]), in fp32.  lo, hi = minimum and maximum of
 *   the tile's finite v (+inf, -inf without one) = ranges[t].  Colour index of a finite v, every operation in fp32 in this order:
 *   u = (v - lo) / ((hi - lo) + 1e-8f), f = floorf(255.0f u), idx = 255 if f >= 255, (int)f if f > 0, else 0 (so a NaN u, inf / inf when
 *   v - lo overflows, gives 0); a non-finite v has idx 0.  Tile t sits at row t / cols, column t % cols, with origin
 *   y0 = pad + (t / cols)(h zoom + pad), x0 = pad + (t % cols)(w zoom + pad); sheet pixel (y0 + i, x0 + j), i < h zoom, j < w zoom, takes the
 *   three bytes luts[ramp][idx(v[i / zoom][j / zoom])].  Every other pixel (gutters, the empty cells of the last row) takes the three
 *   background bytes.  A tile with ia outside 0..Na-1, ib >= Nb or ramp outside 0..L-1 is painted as background and has the range NaN, NaN.
 *   Two launches: one workgroup per tile for the ranges (minimum and maximum are exact: any order), then one thread per four pixels of
 *   the sheet taken as one flat array, three whole 4-byte stores each; no workspace.  Refused before the launch, in this order: a null a,
 *   tiles, luts, ranges or sheet; what pk_plane_sheet_size refuses; Na < 1, Nb < 0, Nb > 0 with b NULL, L < 1; a background value outside
 *   0..255; a, b, tiles, ranges or the sheet not 4-byte aligned.
 * pk_heatmap_quality: pred, gt (M,h,w) fp32; records (M,PK_QUALITY_COLS) float64, every element written.  One 256-thread workgroup per
 *   map (workgroups stride over the maps when M exceeds the grid).  An element takes part iff p and g are both finite; the others are
 *   counted in column 15 and nowhere else; n = the elements that take part.  All arithmetic on the values widened to float64, without FMA.
 *   Every sum: thread r adds its elements r, r + 256, ... in ascending order to 0.0; then the xor butterfly 32, 16, ..., 1 inside each
 *   wave, then wave 0 + wave 1 + wave 2 + wave 3 (pk_heatmap_summary's order).  Columns: 0, 1 sum p, sum g; 2 sum (p - g)^2; 3 max |p - g|
 *   (0 when n = 0); 4, 5, 6 max p, its x, its y by pk_heatmap_summary's rule (replaced iff v > best in fp32, the smallest flat index among
 *   equal maxima, -0 = +0; -inf at (0, 0) without a value above -inf); 7, 8, 9 the same for g; 10, 11, 12 sum (p - mp)(g - mg),
 *   sum (p - mp)^2, sum (g - mg)^2 with mp = column 0 / n, mg = column 1 / n, taken in a second pass over the map; 13, 14 the number of
 *   elements with p >= 0.5f max p AND g >= 0.5f max g, and with either (products and comparisons in fp32), both 0 unless both peaks are
 *   > 0; 15 the elements left out.  Refused before the launch, in this order: a null pointer; M, h or w < 1 or h w > PK_PANEL_MAX_PLANE;
 *   pred or gt not 4-byte or records not 8-byte aligned.                                                                              */
#define PK_PANEL_MAX_TILES 4096
#define PK_PANEL_MAX_SIDE 8192
#define PK_PANEL_MAX_PLANE 16777216
#define PK_PANEL_MAX_ZOOM 64
#define PK_PANEL_MAX_PAD 64
#define PK_QUALITY_COLS 16
int pk_gather_planes(const void* x /* (B,H,W,C) bf16 */, int B, int H, int W, int C, int b, const int32_t* channels /* (n) */, int n, int c_used,
                     float* out /* (n,H,W) */, void* stream);
int pk_plane_sheet_size(int T, int h, int w, int cols, int zoom, int pad, int* SH, int* SW);
int pk_plane_sheet(const float* a /* (Na,h,w) */, int Na, const float* b /* (Nb,h,w) or NULL */, int Nb, const int32_t* tiles /* (T,3) */, int T,
                   const void* luts_u8 /* (L,256,3) */, int L, float* ranges /* (T,2) */, void* sheet_u8 /* (SH,SW,3) */, int h, int w, int cols,
                   int zoom, int pad, int bg0, int bg1, int bg2, void* stream);
int pk_heatmap_quality(const float* pred, const float* gt /* (M,h,w) */, double* records /* (M,16) */, int64_t M, int h, int w, void* stream);


/* ======================= network contractions (bf16 MFMA, fp32 accumulate; NHWC activations) =======================
 * These replace the groups of ATen calls inside the reference's modules; weights are bf16 "compute copies" packed by
 * pk_pack_weights from the fp32 master parameters (which keep the reference's OIHW / (out,in) layouts).            */

/* A5/A6/H1/H2/A4 conv: nn.Conv2d(k=3|1, stride 1|2, padding k/2, bias=False) of models/hrnet.py:24-33,68-79,
 * models/hrformer.py:309-320,548-551, models/fusion_head.py:211-251 (+ their bias'd 1x1 heads).
 * x (B,Hs,Ws,Cin) bf16; w_packed [Cout][k*k][Cin] bf16; out_mode 0: (B,Ho,Wo,Cout) bf16, 1: same fp32,
 * 2: (B,Cout,Ho,Wo) fp32 planes (head outputs).  stats_partial (optional): [pk_conv_stats_tiles(M)][2][Cout] column
 * sums / sums of squares of the fp32 results for train-mode BatchNorm.  dilated_input=1 evaluates the stride-2
 * data-gradient (input rows/cols are the zero-stuffed output gradient; pass flipped weights, mode 1 of pk_pack_weights).
 * act: 0 none, 2 softplus (nn.Softplus of fusion_head.py:250).                                                      */
/* addend (optional, bf16, shape of the output, out_mode 0, no statistics): out = conv(x) + addend.  Used by the data-gradient launch
 * of the first conv of a residual block (hrnet.py:44-52,92-102): the skip connection's gradient is added in the epilogue instead
 * of by a separate elementwise pass over both gradients.                                                                       */
int pk_conv2d_nhwc(const void* x, const void* w_packed, void* out, float* stats_partial, const float* bias,
                   int B, int Hs, int Ws, int Cin, int Cout, int ksize, int stride, int dilated_input, int Ho, int Wo,
                   int act, int out_mode, const void* addend, void* stream);
/* conv -> eval-mode BatchNorm (-> + residual) (-> ReLU) as ONE launch (models/hrnet.py:24-52 / :92-102 in eval mode: the running
 * statistics make the normalisation a per-channel affine map): out = relu?(col_scale[n] * conv(x)[., n] + col_shift[n] + residual),
 * bf16 NHWC in and out, fp32 scale / shift.  Inference only; ksize 1 / 3, stride 1 / 2. */
int pk_conv2d_affine_nhwc(const void* x, const void* w_packed, void* out, const float* col_scale, const float* col_shift,
                          const void* residual, int relu, int B, int Hs, int Ws, int Cin, int Cout, int ksize, int stride, int Ho,
                          int Wo, void* stream);
int pk_conv_stats_tiles(int M);
/* ---- Grouped launches (round 4): the exchange units (models/hrformer.py:420-491 == models/hrnet.py:157-227) are 2-12 small conv + BatchNorm
 * layers per dependency level; each level runs as ONE launch per kernel family.  Descriptor arrays are HOST memory, read before the call
 * returns (they travel in the kernel arguments); every pointer inside is a borrowed device pointer.  At most PK_GROUP_MAX members.       */
#define PK_GROUP_MAX 12
typedef struct PkConvDesc {        /* one pk_conv2d_nhwc (out_mode 0) or pk_conv2d_affine_nhwc problem                                   */
    const void* x; const void* w; void* out;
    float* stats;                  /* [pk_conv_stats_tiles(B*Ho*Wo)][2][Cout] partial statistics, or NULL                                */
    const float* col_scale;        /* eval-mode BatchNorm folded into the epilogue (with bias = shift), or NULL                          */
    const float* bias;
    const void* res;               /* residual (affine form) or addend (data gradient), bf16, shape of out, or NULL                      */
    int B, Hs, Ws, Cin, Cout, ksize, stride, dilated_input, Ho, Wo;
    int act;                       /* 0 none, 3 ReLU after the residual add                                                              */
} PkConvDesc;
int pk_conv2d_group(const PkConvDesc* descs, int n, void* stream);
typedef struct PkBnFwdDesc {       /* one pk_bn_train_fwd problem (finalize + apply in one pass; any row count)                          */
    const void* raw; const float* stats_partial; const float* gamma; const float* beta;
    float* running_mean; float* running_var; int64_t* num_batches_tracked;
    const void* residual; void* y; float* save_mean; float* save_rstd; uint8_t* relu_mask /* optional, see pk_bn_act */;
    int64_t rows; int tiles, C; float momentum, eps; int relu;
} PkBnFwdDesc;
int pk_bn_train_fwd_group(const PkBnFwdDesc* descs, int n, void* stream);
typedef struct PkBnBwdDesc {       /* one pk_bn_bwd problem; partial: [pk_bn_bwd_group_blocks(rows)][2][C] floats                        */
    const void* dy; const void* y_act; const void* raw; const float* save_mean; const float* save_rstd; const float* gamma;
    float* partial; float* dgamma; float* dbeta; void* dx; void* dresidual; const uint8_t* relu_mask /* optional: replaces y_act */;
    int64_t rows; int C; int relu;  /* bit 0: mask by relu_mask / y_act > 0; bit 1: eval-mode statistics (no batch-mean terms)               */
} PkBnBwdDesc;
int pk_bn_bwd_group_blocks(int64_t rows);
int pk_bn_bwd_group(const PkBnBwdDesc* descs, int n, void* stream);
typedef struct PkFuseDesc {        /* one pk_fuse_sum problem; mask_y (optional, shape of out): input 0 counts only where mask_y > 0 (the ReLU
                                    * backward of a fused sum folded into the sum of input gradients)                                      */
    const void* inputs[4]; int in_h[4]; int in_w[4]; int n_inputs;
    void* out; const void* mask_y; int B, H, W, C, relu;
} PkFuseDesc;
int pk_fuse_sum_group(const PkFuseDesc* descs, int n, void* stream);
typedef struct PkUpBwdDesc {       /* one pk_upsample_bilinear_bwd problem; mask_y (optional, shape of dy): dy counts only where mask_y > 0  */
    const void* dy; const void* mask_y; void* dsrc; int B, H, W, Hs, Ws, C;
} PkUpBwdDesc;
int pk_upsample_bwd_group(const PkUpBwdDesc* descs, int n, void* stream);
typedef struct PkWgradDesc {       /* weight-gradient SLABS of one 1x1 stride-1 or 3x3 stride-2 conv (all members of one kind): workspace =
                                    * pk_wgrad_group_slices(...) x N x k*k x Cin floats, layout [S][N][k*k][Cin], reduced by pk_reduce_many */
    const void* x; const void* grad_out; float* workspace;
    int B, Hs, Ws, Ho, Wo, N, Cin, ksize, stride;
} PkWgradDesc;
int pk_wgrad_group_slices(int M, int N, int Cin, int ksize, int stride);
int pk_wgrad_group(const PkWgradDesc* descs, int n, void* stream);
int pk_sizeof_group_desc(int which);   /* sizeof of PkConvDesc (0), PkBnFwdDesc (1), PkBnBwdDesc (2), PkFuseDesc (3), PkUpBwdDesc (4), PkWgradDesc (5) */

/* Rows of the [rows][2][Cout] partial-statistics buffer a pk_conv2d_nhwc launch with bf16 output and statistics writes for this geometry
 * (the 3x3 halo kernel emits one row per 64 padded positions; everything else pk_conv_stats_tiles(B*Ho*Wo)).  Replaces the per-call
 * `torch.var_mean` inside nn.BatchNorm2d of the reference (models/hrnet.py:24-52): pk_bn_finalize sums the rows it is given. */
int pk_conv_stats_rows(int B, int Hs, int Ws, int Cin, int Cout, int ksize, int stride, int Ho, int Wo);

/* A1/A3 linear layers: nn.Linear qkv/proj (models/hrformer.py:167-169,180,197) and Mlp fc1/fc2 (:53-55,58-64).
 * out[o_rowmap[m]] = residual + res_scale[sample] * act(x[a_rowmap[m]] @ w^T + bias).  Row maps implement
 * window_partition / window_reverse (hrformer.py:67-114) inside the GEMM: a_rowmap -1 = zero pad token, o_rowmap -1 =
 * cropped token.  act 1 = exact-erf GELU (nn.GELU, hrformer.py:54).  preact_out saves the pre-GELU values;
 * gelu_grad_of multiplies the result by gelu'(z) (backward through the activation).                                  */
int pk_linear_bf16(const void* x, const void* w, void* out, const float* bias, const void* residual, const float* res_scale,
                   const int32_t* a_rowmap, const int32_t* o_rowmap, void* preact_out, const void* gelu_grad_of,
                   int M, int N, int K, int rows_per_sample, int act, int out_fp32, void* stream);

/* A2 as stand-alone functions: window_partition / window_reverse (models/hrformer.py:67-114) move whole rows through the window row map
 * (window-order token -> pixel row, -1 = zero token appended at the bottom / right).  scatter 0: dst[r] = src[rowmap[r]] (or zeros) =
 * partition; scatter 1: dst[rowmap[r]] = src[r] where rowmap[r] >= 0 = reverse + crop.  Any element type, rows of whole dwords.
 * drop_path (hrformer.py:15-24): out = (x / keep_prob) * mask[sample], fp32.                                                          */
int pk_rows_by_map(const void* src, void* dst, const int32_t* rowmap, int64_t n_rows, int row_bytes, int scatter, void* stream);
int pk_drop_path_f32(const float* x, const float* mask, float* out, int64_t batch, int64_t per_sample, float keep_prob, void* stream);

/* weight gradient of either form: dw = sum_m grad_out[m]^T (x) A(m); workspace = pk_wgrad_slices(...)*N*(k*k*Cin + 1) floats.
 * out_layout 0: [N][k*k][Cin]; 1: OIHW (the reference's nn.Conv2d.weight layout).  Ho == 0 selects the linear form.
 * dbias (optional, n_bias <= N entries): the bias gradient = column sums of the same (gathered, scaled) grad_out rows,
 * accumulated from the tile already staged in LDS.                                                                       */
/* Row maps (linear form): a_rowmap / g_rowmap give the source row of x / grad_out for GEMM row m (-1 = zero row); g_scale multiplies
 * grad_out row r by g_scale[r / g_rows_per_sample] (DropPath).  When the maps are the 7x7 WINDOW PARTITION of a (B, Hs, Ws) token
 * grid (nnops.window_rowmap: m = ((b*nh + wy)*nw + wx)*49 + ty*7 + tx -> pixel (wy*7+ty, wx*7+tx), pad tokens -1), pass B, Hs, Ws
 * with Ho = Wo = 0: the streaming kernel then RECOMPUTES the map per DMA lane instead of loading it (M must equal B*nh*nw*49, and
 * g_rows_per_sample must be Hs*Ws).  With B = Hs = Ws = 0 the map is loaded (any map, slower kernel).                          */
/* dw == NULL: write the slabs only (weight slabs [S][N*k*k*Cin], then bias slabs [S][N] when n_bias > 0) and let the caller
 * reduce them later with pk_reduce_many.                                                                                  */
/* pk_wgrad_slices: the slab count S of the launch pk_wgrad_bf16 will make for the same arguments (Hs = Ws = 0 for the linear
 * form; flags bit 0 = a_rowmap given, bit 1 = g_rowmap given, bit 2 = g_scale given).                                         */
int pk_wgrad_slices(int M, int N, int Cin, int ksize, int stride, int Hs, int Ws, int flags);
int pk_wgrad_bf16(const void* x, const void* grad_out, float* workspace, float* dw, float* dbias, int n_bias,
                  const int32_t* a_rowmap, const int32_t* g_rowmap, const float* g_scale, int g_rows_per_sample, int M, int N,
                  int Cin, int ksize, int stride, int B, int Hs, int Ws, int Ho, int Wo, int out_layout, void* stream);

/* window attention core (models/hrformer.py:183-196): softmax(scale*q k^T + table[index]) v per (window, head);
 * qkv (n_windows*49, 3C) bf16 in the reference's channel order s*C + h*d + e; rel_table (169, heads) fp32.          */
/* head_dim d = C/heads: multiple of 8, <= 64.  softmax_scale <= 0 selects the reference's d^-0.5 (hrformer.py:140); a
 * caller that pads 39-wide heads to 40 passes 39^-0.5 explicitly.                                                        */
int pk_window_attn_fwd(const void* qkv, const float* rel_table, void* out, float* lse, int n_windows, int heads, int C,
                       float softmax_scale, void* stream);
int pk_window_attn_bwd_groups(int n_windows, int heads);
int pk_window_attn_bwd_ws_floats(int n_windows, int heads);  /* size of dbias_partial in floats */
/* fwd_out = the `out` tensor pk_window_attn_fwd produced for the same qkv (delta_i = sum_e dout[i][e] * out[i][e]). */
int pk_window_attn_bwd(const void* qkv, const float* rel_table, const void* fwd_out, const void* dout, const float* lse, void* dqkv,
                       float* dbias_partial, float* dtable, int n_windows, int heads, int C, float softmax_scale, void* stream);

/* ======================= normalisation / elementwise (HBM-bound, NHWC bf16, 16 bytes per lane) ==================== */
int pk_sum_partials(const float* partial, int nb, int K, int stride, float* out, float scale, int accumulate, void* stream);
/* nn.BatchNorm2d train mode (eps 1e-5, momentum 0.1, unbiased running_var): finalize conv-epilogue sums -> scale/shift */
int pk_bn_finalize(const float* stats_partial, int tiles, int C, int count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                   float* scale, float* shift, float* save_mean, float* save_rstd, void* stream);
/* relu_mask (optional, rows*C/8 bytes): one byte per 16-byte chunk of y, bit j = channel j of the chunk is > 0 after the ReLU.  The
 * backward kernels read it instead of the activated output (1/16 of the bytes).                                                    */
int pk_bn_act(const void* x, const float* scale, const float* shift, const void* residual, void* y, int64_t rows, int C,
              int relu, uint8_t* relu_mask, void* stream);   /* y = relu?(x*scale + shift (+ residual)) */
/* Train-mode BatchNorm forward from the conv epilogue's partial statistics (nn.BatchNorm2d.forward in models/hrnet.py:24-52,
 * models/hrformer.py:309-344): pk_bn_finalize + pk_bn_act, as ONE launch for small tensors (tiles <= 128).  scale / shift: [C] workspaces. */
int pk_bn_train_fwd(const void* raw, const float* stats_partial, int tiles, int C, int64_t rows, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps, const void* residual,
                    void* y, float* save_mean, float* save_rstd, float* scale, float* shift, int relu, uint8_t* relu_mask, void* stream);
int pk_bn_bwd_blocks(int64_t rows);                          /* partial needs blocks*2*C floats */
/* pk_bn_bwd `relu`: bit 0 = the forward applied ReLU (mask from relu_mask when given, else from y_act); bit 1 = eval-mode BatchNorm (save_mean / save_rstd hold the
 * running statistics, which are constants: dx = gamma * rstd * g, no batch-mean terms; dgamma / dbeta as in training).           */
int pk_bn_bwd(const void* dy, const void* y_act, const void* raw, const float* save_mean, const float* save_rstd,
              const float* gamma, float* partial, float* sums, float* dgamma, float* dbeta, void* dx, void* dresidual,
              int64_t rows, int C, int relu, const uint8_t* relu_mask, void* stream);
int pk_relu_bwd(const void* dy, const void* y, void* dx, int64_t numel, void* stream);

/* ---- 1x1 convolution 64 -> 256 + BatchNorm with the pre-normalisation tensor recomputed, never stored (pk_conv1x1_bn.hip): layer1's
 * conv3 + bn3 and downsample branch (models/_blocks.py).  x: [rows][64] bf16, w: the packed forward weight [256][1][64] bf16; every
 * 256-channel tensor [rows][256] bf16; all of them 16-byte aligned.  bf16(x w^T) is bit for bit what pk_conv2d_nhwc stores.
 * pk_conv1x1_bn_supported: 1 for Cin = 64, Cout = 256, rows >= 32 768 (where pk_bn_train_fwd / pk_bn_bwd take their large-tensor form).
 *   Per-call environment switches: PK_CONV1X1_BN=0 (route off), PK_CONV1X1_BN_MIN_ROWS (row threshold), PK_CONV1X1_BN_MAX_GRID (at most
 *   this many workgroups per launch).
 * pk_conv1x1_stats: the statistics-only pass: stats_partial [pk_conv1x1_stats_rows(rows)][2][Cout] sums / sums of squares of the fp32
 *   accumulators per 128 rows, what pk_bn_finalize reads.
 * pk_conv1x1_bn_act: y = relu?(bf16(conv) * scale + shift (+ residual)) and the ReLU bit mask, as pk_bn_act computes them from a stored raw.
 * pk_conv1x1_bn_bwd: pk_bn_bwd (training mode; relu needs relu_mask) with (x, w) in place of raw: _bwd_reduce writes partial
 *   [pk_conv1x1_bn_bwd_rows(rows)][2][Cout] (= pk_bn_bwd_blocks(rows): pk_bn_bwd's own partial rows, bit for bit), their fixed-order sum
 *   goes to sums [2][Cout] and dbeta / dgamma, _bwd_apply writes draw and the optional dresidual; above 32 768 rows every output equals
 *   pk_bn_bwd's on the stored raw bit for bit.                                                                                                          */
int pk_conv1x1_bn_supported(int64_t rows, int Cin, int Cout);
int pk_conv1x1_stats_rows(int64_t rows);
int pk_conv1x1_bn_bwd_rows(int64_t rows);
int pk_conv1x1_stats(const void* x, const void* w, float* stats_partial, int64_t rows, int Cin, int Cout, void* stream);
int pk_conv1x1_bn_act(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y, int relu,
                      uint8_t* relu_mask, int64_t rows, int Cin, int Cout, void* stream);
int pk_conv1x1_bn_bwd_reduce(const void* dy, const void* x, const void* w, const float* save_mean, const float* save_rstd, float* partial,
                             int64_t rows, int Cin, int Cout, int relu, const uint8_t* relu_mask, void* stream);
int pk_conv1x1_bn_bwd_apply(const void* dy, const void* x, const void* w, const float* save_mean, const float* save_rstd, const float* gamma,
                            const float* sums, float inv_count, void* draw, void* dresidual, int64_t rows, int Cin, int Cout, int relu,
                            const uint8_t* relu_mask, void* stream);
int pk_conv1x1_bn_bwd(const void* dy, const void* x, const void* w, const float* save_mean, const float* save_rstd, const float* gamma,
                      float* partial, float* sums, float* dgamma, float* dbeta, void* draw, void* dresidual, int64_t rows, int Cin, int Cout,
                      int relu, const uint8_t* relu_mask, void* stream);
/* ---- BatchNorm (train) + ReLU + 1x1 output conv of a fusion-head branch; the output conv's data gradient dt is never stored and the
 * activated tensor t is written but not read back in forward (pk_bn_out1x1.hip).  raw, t: [rows][C] bf16, C = 128 or 256; N <= 48
 * outputs; rows = B * hw.
 * pk_bn_out1x1_supported: 1 for those shapes at rows >= 32 768.  Per-call environment switches: PK_BN_OUT1X1=0 (route off),
 *   PK_BN_OUT1X1_MIN_ROWS (row threshold), PK_BN_OUT1X1_MAX_GRID (at most this many workgroups per launch).
 * pk_bn_out1x1_fwd: t = bf16(relu(raw * scale + shift)), the ReLU bit mask and out [B][N][hw] fp32 = conv1x1(t) + bias (softplus): bit for
 *   bit pk_bn_act followed by pk_conv2d_nhwc (out_mode 2).  w_fwd: the packed forward weight [N][1][C].
 * pk_bn_out1x1_bwd: g = the maps' gradient as [rows][up8(N)] bf16 (pk_nchw_f32_to_nhwc_bf16, channels >= N zero); w_dgrad: the packed
 *   data-gradient weight [C][1][up8(N)].  dt = bf16(g w_dgrad^T) is recomputed in both passes: partial [pk_bn_bwd_blocks(rows)][2][C],
 *   sums [2][C], dgamma, dbeta and draw are pk_bn_bwd's on a stored dt bit for bit (either of its forms).                              */
int pk_bn_out1x1_supported(int64_t rows, int C, int N);
int pk_bn_out1x1_fwd(const void* raw, const float* scale, const float* shift, const void* w_fwd, const float* bias, void* t, float* out,
                     uint8_t* relu_mask, int64_t rows, int C, int N, int hw, int softplus, void* stream);
int pk_bn_out1x1_bwd(const void* g, const void* raw, const uint8_t* relu_mask, const void* w_dgrad, const float* save_mean,
                     const float* save_rstd, const float* gamma, float* partial, float* sums, float* dgamma, float* dbeta, void* draw,
                     int64_t rows, int C, int N, void* stream);
/* nn.LayerNorm(C, eps 1e-5) over the channel dim of NHWC rows (hrformer.py:240,252,273,288).  C = row width (multiple of 8,
 * <= 1024); C_real (0 = C) = number of real channels when the rows carry zero padding: statistics over the real channels,
 * padded outputs / input gradients are zero.  gamma/beta (and dgamma/dbeta) have C entries, 16-byte aligned; the padded
 * entries are ignored.                                                                                                  */
int pk_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* save_mean, float* save_rstd,
                     int64_t rows, int C, int C_real, float eps, void* stream);
int pk_ln_bwd_blocks(int64_t rows);                          /* partial needs blocks*2*C floats */
int pk_layernorm_bwd(const void* dy, const void* x, const float* save_mean, const float* save_rstd, const float* gamma,
                     const void* dresidual, void* dx, float* partial, float* dgamma, float* dbeta, int64_t rows, int C, int C_real,
                     void* stream);
/* Fused MLP half of the HRFormer block (hrformer.py:288-291 with Mlp :38-64 and DropPath :15-35), C = 32 / 64:
 *   y = x + row_scale[b] * ( fc2( gelu_erf( fc1( LayerNorm(x; gamma, beta, eps) ) + b1 ) ) + b2 )       x, y: [M][C] bf16
 * ONE launch; the 4C-wide hidden activation stays in registers.  w1 = fc1.weight [4C][C] bf16, w2 = fc2.weight [C][4C] bf16
 * (forward copies); w1_t = [C][4C], w2_t = [4C][C] (data-gradient copies).  row_scale (or NULL) is indexed by row / rows_per_sample.
 * Backward recomputes LayerNorm / fc1 / GELU from x (nothing but x is saved):
 *   pk_ln_mlp_bwd_dx: dx = dy + dLayerNorm(...), ln_partial[pk_ln_mlp_dx_blocks][2][C] = per-workgroup sums for dgamma | dbeta;
 *   pk_ln_mlp_bwd_dw: slabs[(4C / HS) slices][pk_ln_mlp_dw_blocks][pk_ln_mlp_slab_floats] with HS = pk_ln_mlp_hidden_slice(C);
 *                     one slab = [ dW1 rows h0..h0+HS [HS][C] | dW2 columns h0..h0+HS [C][HS] | db1[h0..] [HS] | db2 [C] ] fp32,
 *                     to be summed over the workgroup index (pk_reduce_many layouts 0 / 2); db2 is complete in every slice.   */
int pk_ln_mlp_supported(int C);
int pk_ln_mlp_hidden_slice(int C);
int pk_ln_mlp_slab_floats(int C);
int pk_ln_mlp_dx_blocks(int M, int C);
int pk_ln_mlp_dw_blocks(int M, int C);
int pk_ln_mlp_fwd(const void* x, const float* gamma, const float* beta, const void* w1, const float* b1, const void* w2,
                  const float* b2, const float* row_scale, void* y, int M, int C, int rows_per_sample, float eps, void* stream);
/* The same half for wide channels (C = 80 / 128 / 160 / 256 / 320; hrformer.py:262-293 with Mlp :38-64 at stage-3/4 widths and the
 * 8-aligned twin of HRFormer-base :779-825), forward only: fc1 / fc2 weights streamed through LDS in hidden slices of 32.  `c_real` <= C:
 * channels the LayerNorm statistics run over (the padded channels hold zeros).  w1 [hidden][C], w2 [C][hidden] bf16 row-major. */
int pk_ln_mlp_wide_supported(int C, int hidden, int M);   /* M > 0: ... and the launch has enough workgroups to pay (M = 0: built for?) */
int pk_ln_mlp_wide_fwd(const void* x, const float* gamma, const float* beta, const void* w1, const float* b1, const void* w2,
                       const float* b2, const float* row_scale, void* y, int M, int C, int c_real, int hidden, int rows_per_sample,
                       float eps, void* stream);
int pk_ln_mlp_bwd_dx(const void* dy, const void* x, const float* gamma, const float* beta, const void* w1, const float* b1,
                     const void* w1_t, const void* w2_t, const float* row_scale, void* dx, float* ln_partial, int M, int C,
                     int rows_per_sample, float eps, void* stream);
int pk_ln_mlp_bwd_dw(const void* dy, const void* x, const float* gamma, const float* beta, const void* w1, const float* b1,
                     const void* w2_t, const float* row_scale, float* slabs, int M, int C, int rows_per_sample, float eps,
                     void* stream);
/* Attention half for the 8-aligned twin of HRFormer-base (hrformer.py:779-825: C = heads x 39, here heads x 40 with zero padding; block
 * :262-286, WindowAttention :174-200), forward only: C = 80 with 2 heads.  wqkv [3][heads][40][C], wproj [C][heads][40] bf16, biases and
 * LayerNorm parameters zero in the padded entries; `c_real` = channels the LayerNorm statistics run over, `softmax_scale` = real
 * head_dim^-0.5.  `n_windows` > 0 in _supported additionally asks whether the launch has enough windows to pay. */
int pk_attn_block_wide_supported(int C, int heads, int n_windows);
int pk_attn_block_wide_fwd(const void* x, const int32_t* rowmap, const float* gamma, const float* beta, const float* rel_table,
                           const void* wqkv, const float* bqkv, const void* wproj, const float* bproj, const float* row_scale,
                           void* y, int n_windows, int windows_per_sample, int heads, int C, int c_real, float softmax_scale,
                           float eps, void* stream);
/* Fused attention half of the HRFormer block (hrformer.py:262-286 with WindowAttention :174-200, window_partition/reverse :67-114),
 * C = 32 / 64, head_dim 32, window 7:   y = x + row_scale[b] * proj( attention( qkv( LayerNorm(x) ) ) )     x, y: [M][C] bf16 pixel rows.
 * rowmap[windows*49]: pixel row of every window token, -1 for the reference's zero-pad tokens (LayerNorm output forced to 0, i.e.
 * q = b_q, k = b_k, v = b_v; attended without a mask, output dropped).  o_save ([windows*49][C] bf16) and lse ([windows][heads][49])
 * may be NULL (inference); training saves them for pk_attn_block_bwd.  row_scale is indexed by window / windows_per_sample.     */
int pk_attn_block_supported(int C, int heads);
int pk_attn_block_fwd(const void* x, const int32_t* rowmap, const float* gamma, const float* beta, const float* rel_table,
                      const void* wqkv, const float* bqkv, const void* wproj, const float* bproj, const float* row_scale,
                      void* y, void* o_save, float* lse, int n_windows, int windows_per_sample, int heads, int C, float eps,
                      void* stream);
/* Backward of the fused attention half: dx = dy + dLayerNorm(dqkv W_qkv) written to the pixel rows (pad tokens dropped); emits
 * dqkv [windows*49][3C] bf16 and the LayerNorm output u in window order [windows*49][C] (zero rows at the pad tokens) for the
 * weight-gradient GEMMs (pk_wgrad_bf16: dW_qkv = dqkv^T u, dW_proj = (s dy)^T o), ln_partial[pk_attn_block_blocks][2][C]
 * (dgamma | dbeta sums) and rpb_partial[pk_attn_block_blocks*4][heads][169] (rel-pos-bias gradient per wave).  wqkv_t = [C][3C],
 * wproj_t = [C][C] data-gradient copies; o_saved / lse from pk_attn_block_fwd.                                                */
int pk_attn_block_blocks(int n_windows);
int pk_attn_block_bwd(const void* dy, const void* x, const int32_t* rowmap, const float* gamma, const float* beta,
                      const float* rel_table, const void* wqkv, const float* bqkv, const void* wqkv_t, const void* wproj_t,
                      const float* row_scale, const void* o_saved, const float* lse, void* dx, void* dqkv, void* u_out,
                      float* ln_partial, float* rpb_partial, int n_windows, int windows_per_sample, int heads, int C, float eps,
                      void* stream);
int pk_colsum_bf16(const void* g, const int32_t* rowmap, const float* row_scale, int rows_per_sample, float* partial,
                   float* out, int64_t rows, int N, void* stream);
/* exchange unit sum (hrformer.py:471-489 == hrnet.py:207-225): out = relu?(sum_i bilinear_up_i(x_i)), F.interpolate
 * (mode='bilinear', align_corners=False) fused into the sum; and the up-sampling backward in gather form.            */
int pk_fuse_sum(const void* const* inputs, const int* in_h, const int* in_w, int n_inputs, void* out, int B, int H, int W,
                int C, int relu, void* stream);
int pk_upsample_bilinear_bwd(const void* dy, void* dsrc, int B, int H, int W, int Hs, int Ws, int C, void* stream);
int pk_nchw_f32_to_nhwc_bf16(const float* x, const float* softplus_out, void* y, int B, int Cin, int H, int W, int Cpad,
                             void* stream);   /* softplus_out != NULL: also multiply by d softplus/dz = 1-exp(-y) */
/* fp32 master weights -> bf16 compute copies, table driven, one launch for the whole model (see nnops.WeightCache).
 * desc_table: array of {const float* src; int64 dst_off; int N,C,T,mode,Cp,Np; int64 dst_numel} (48 bytes each);
 * mode 0: dst[n][t][cp]=src[n][c][t] (forward), 1: dst[c][T-1-t][np]=src[n][c][t] (conv data-grad), 2: dst[c][np]=src[n][c] */
/* Deferred parameter-gradient reductions: ONE launch for any number of slab sums  out[index(i)] = sum_{s<S} part[s*slab_stride + i], i < K.
 * desc_table rows (56 bytes): { const float* part; float* out; int64 slab_stride; int S, K, layout, N, T, Cin, out_stride, pad; };
 * layout 0: index(i) = i*out_stride; layout 1: i = (n*T + t)*Cin + c -> OIHW (n*Cin + c)*T + t; layout 2: i = a*Cin + b -> a*T + b*out_stride.  One 256-thread block per
 * pk_reduce_many_cols() outputs (block_desc = row, block_first = first block of that row).  Producers: pk_wgrad_bf16 (dw NULL), pk_layernorm_bwd
 * (dgamma/dbeta NULL: partial is [blocks][2C]), pk_window_attn_bwd (dtable NULL: partial is [groups][169]).                   */
int pk_reduce_many_cols(void);
int pk_reduce_many(const void* desc_table, const int* block_desc, const int* block_first, int n_blocks, void* stream);
int pk_pack_weights(void* flat_dst_bf16, const void* desc_table, const int32_t* block_desc, const int32_t* block_first,
                    int n_blocks, void* stream);
/* Padded twins (models whose channel counts are not multiples of 8, e.g. HRFormer-base C=78, head_dim 39 -- hrformer.py:779-825):
 * every real fp32 tensor is a box r[4] at the origin of the twin's box p[4] inside one flat twin buffer.
 * desc_table rows (56 bytes): { float* real; int64 twin_off; int r[4]; int p[4]; int64 numel; }; one 256-thread block per
 * 1024 real elements (block_desc = row index, block_first = first block of that row).
 * direction 0: twin <- real (parameters, buffers); 1: real <- twin (gradients into a sink, BatchNorm running statistics);
 * 2: real += twin (accumulate into .grad).                                                                              */
int pk_embed_boxes(float* twin_base, const void* desc_table, const int* block_desc, const int* block_first, int n_blocks,
                   int direction, void* stream);

/* Pose overlays (utils/visualization.py), drawn in place on a uint8 batch images (N,H,W,3), H, W <= 8192.
 * pk_draw_shapes: boxes (Q,4) fp32 x1 y1 x2 y2 with box_image_index (Q,), one colour (channel order of the image) and thickness; then
 *   poses (P,K,2) fp32 image pixels, scores (P,K), image_index (P,); both index tables non-decreasing.  limbs (L,2) int32 (a limb naming
 *   a joint outside 0..K-1 is skipped), colors (C,3) uint8 (joint k and limbs starting at k take colors[k % C]).  Coverage is decided
 *   in integers on 16 samples per pixel in units of 1/8 px (rule: DESIGN.md "Drawing on the device"); per image boxes first, then per
 *   pose limbs in table order and joints in index order (disc, white ring), drawn iff score >= score_threshold and everything finite.
 *   point_radius 0..64, line_thickness / box_thickness 1..64.  No atomics: identical bits on every run.
 * pk_heatmap_overlay: heatmaps (N,K,h,w) fp32 -> max over K, bilinear resize to (H,W) (half-pixel rule), per-image min/max of the
 *   resized plane, idx = floor(255 (m - min) / (max - min + 1e-8)), out = (img (256 - a) + lut[idx] a + 128) >> 8 with
 *   a = clamp(rint(256 alpha), 0, 256).  lut: (256,3) uint8; index_u8 (optional): (N,H,W) uint8 receives idx;
 *   ws: pk_heatmap_overlay_ws_floats(...) floats.
 * pk_heatmap_overlay_patches: one stack per person.  heatmaps (P,K,h,w) fp32; patch_image_index (P,) int32 non-decreasing, each in
 *   [0, N) (NOT checked here: the caller guarantees it; a frame may have none or many); patch_matrix (P,6) float64 on the device, the
 *   2x3 map from frame pixels to heat-map pixels (the crop matrix with (w,h) as its output size).  m_p = max over K, lo_p / hi_p =
 *   min / max of m_p over its own plane; frame pixel (X,Y) is covered by p iff (s,t) = M_p (X,Y,1) (float64) has 0 <= s <= w-1 and
 *   0 <= t <= h-1; v = max over the covering p of (bilinear(m_p; s,t) - lo_p) / (hi_p - lo_p + 1e-8); idx = clamp(floor(255 v)), NaN -> 0;
 *   covered pixels get the blend of pk_heatmap_overlay, the others keep their bytes.  index_u8 / cover_u8 (optional): (N,H,W) uint8
 *   receive idx (0 where uncovered) and the number of covering patches (saturating at 255).  P <= 65535.  No atomics.
 *   ws: pk_heatmap_overlay_patches_ws_floats(...) floats.                                                                            */
int pk_draw_shapes(void* images_u8, int N, int H, int W, const float* poses, const float* scores, const int32_t* image_index, int P,
                   int K, const int32_t* limbs, int L, const void* colors_u8, int C, const float* boxes,
                   const int32_t* box_image_index, int Q, int box_c0, int box_c1, int box_c2, int box_thickness,
                   float score_threshold, int point_radius, int line_thickness, void* stream);
int pk_heatmap_overlay_ws_floats(int N, int K, int h, int w, int H, int W);
int pk_heatmap_overlay(void* images_u8, const float* heatmaps, float alpha, const void* lut_u8, void* index_u8, float* ws, int N,
                       int K, int h, int w, int H, int W, void* stream);
int pk_heatmap_overlay_patches_ws_floats(int P, int K, int h, int w);
int pk_heatmap_overlay_patches(void* images_u8, const float* heatmaps, const int32_t* patch_image_index, const double* patch_matrix,
                               float alpha, const void* lut_u8, void* index_u8, void* cover_u8, float* ws, int N, int P, int K, int h,
                               int w, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POSEKERNELS_H */
