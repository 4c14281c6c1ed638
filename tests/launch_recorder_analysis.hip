// Host-only launch recorder for the analysis units (tests/test_launch_routes_analysis.py): the ten launching entries and the three
// workspace queries of pk_motion.hip (pk_pck, pk_motion_stats, pk_position_histogram), pk_spectrum.hip, pk_nms.hip (pk_pose_rescore,
// pk_oks_nms), pk_eval.hip (pk_coco_kpt_oks, pk_coco_kpt_eval) and pk_draw.hip, swept over the smallest values at which each launch rule
// or argument check can go wrong.  One line per call: the problem, every launch (kernel, grid, block, LDS bytes, every argument:
// pointers as the made-up addresses, floats as hex floats, every field of k_draw_shapes' argument struct), the return code and the
// error text as pk_last_error_string gives it back (the library's own error state is compiled in).
//
// Build: hipcc --offload-host-only -O1 -std=c++17 -w tests/launch_recorder_analysis.hip -o launch_recorder_analysis
// -DPK_ANALYSIS_CSRC=/path/to/csrc records from the units of another tree (its include/ two levels above csrc/, as here).
#define REC_LIBRARY_ERRORS
#include "launch_recorder.h"

#include <math.h>

#include <type_traits>

#ifndef PK_ANALYSIS_CSRC
#define PK_ANALYSIS_CSRC ../infantposeestimation_gaussianbias_amd/csrc
#endif
#define REC_STR2(x) #x
#define REC_STR(x) REC_STR2(x)
#define REC_UNIT(name) REC_STR(PK_ANALYSIS_CSRC/name)
#include REC_UNIT(pk_status.hip)
#include REC_UNIT(pk_motion.hip)
#include REC_UNIT(pk_spectrum.hip)
#include REC_UNIT(pk_nms.hip)
#include REC_UNIT(pk_eval.hip)
#include REC_UNIT(pk_draw.hip)

// ---- argument printers
static void rec_struct(const DrawArgs& a) {
    emit(" {%lx %d %d %d %lx %lx %lx %d %d %lx %d %lx %d %lx %lx %d %x %d %a %d %d %d}", (unsigned long)(uintptr_t)a.img, a.N, a.H, a.W,
         (unsigned long)(uintptr_t)a.poses, (unsigned long)(uintptr_t)a.scores, (unsigned long)(uintptr_t)a.pose_img, a.P, a.K,
         (unsigned long)(uintptr_t)a.limbs, a.L, (unsigned long)(uintptr_t)a.colors, a.C, (unsigned long)(uintptr_t)a.boxes,
         (unsigned long)(uintptr_t)a.box_img, a.Q, a.box_color, a.box_half, (double)a.thr, a.r0, a.r1, a.half);
}
template <class T> static void rec_val(const T& v) {
    if constexpr (std::is_pointer_v<T>) emit(" %lx", (unsigned long)(uintptr_t)v);
    else if constexpr (std::is_floating_point_v<T>) emit(" %a", (double)v);
    else if constexpr (std::is_integral_v<T>) emit(" %lld", (long long)v);
    else rec_struct(v);
}
template <class... A> static void rec_args(Rec, const A&... a) {
    emit(" a=");
    (rec_val(a), ...);
}

// ---- made-up addresses, one region per argument position; `null_at` knocks one pointer out (0-based, -1: none)
struct Ptrs {
    int null_at;
    void* operator()(int k) const { return k == null_at ? nullptr : fake<void>(0x10000000u + 0x08000000u * (uintptr_t)k); }
    template <class T> T* f(int k) const { return (T*)(*this)(k); }
};
static const Ptrs kGood{-1};
static Ptrs null_at(int k) { return Ptrs{k}; }
template <class Call> static void each_null(int n, Call call) {
    for (int k = 0; k < n; ++k) call(null_at(k));
}
static void tag(const Ptrs& P) { emit(" null=%d", P.null_at); }
static void done(int rc) {
    finish(rc);
    flush_line();
}
static const int kBig = 46341;          // kBig * kBig is the first square above 2^31
static const int kMax = 0x7fffffff;

// ---- pk_motion.hip: one workgroup per joint / per (sequence, joint)
static void pck_call(int N, int K, int n_thr, const Ptrs& P) {
    emit("pck N=%d K=%d n_thr=%d", N, K, n_thr);
    tag(P);
    done(pk_pck(P.f<float>(0), P.f<float>(1), P.f<float>(2), P.f<float>(3), P.f<float>(4), P.f<int64_t>(5), P.f<int64_t>(6), P.f<double>(7), N, K, n_thr,
                STREAM));
}
static void stats_call(int S, int T, int K, float min_conf, const Ptrs& P) {
    emit("motion_stats S=%d T=%d K=%d min_conf=%a", S, T, K, (double)min_conf);
    tag(P);
    done(pk_motion_stats(P.f<float>(0), P.f<float>(1), P.f<double>(2), S, T, K, min_conf, STREAM));
}
static void hist_call(int S, int T, int K, int nbx, int nby, const Ptrs& P) {
    emit("position_histogram S=%d T=%d K=%d nbx=%d nby=%d", S, T, K, nbx, nby);
    tag(P);
    done(pk_position_histogram(P.f<float>(0), P.f<float>(1), P.f<double>(2), P.f<double>(3), P.f<int32_t>(4), S, T, K, nbx, nby, 0.25f, STREAM));
}
// (S, T, K) of the three sequence entries: 1 and 34 joints, S K at 2^31 - 1 and beyond it, each count at 0 and below
static const int kSTK[][3] = {{1, 1, 1},       {2, 300, 34},     {3, 257, 17},        {kMax, 4, 1},  {1, 4, kMax},  {65536, 4, 32767}, {65536, 4, 32768},
                              {kBig, 4, kBig}, {kMax, 4, kMax},  {0, 300, 17},        {2, 0, 17},    {2, 300, 0},   {-1, 300, 17},     {2, -1, 17},
                              {2, 300, -1},    {2, kMax, 17}};
static void sweep_motion() {
    for (int K : {1, 17, 34, 65535, 65536, 0, -1}) pck_call(1000, K, 3, kGood);
    for (int N : {1, 255, 256, 257, kMax, 0, -1}) pck_call(N, 17, 3, kGood);
    for (int n_thr : {1, 2, 16, 17, 0, -1}) pck_call(1000, 17, n_thr, kGood);
    each_null(8, [](const Ptrs& P) { pck_call(1000, 17, 3, P); });
    pck_call(0, 17, 3, null_at(4));             // two faults at once: null thresholds, bad shape
    pck_call(1000, 0, 17, kGood);               // bad shape, too many thresholds

    for (auto& s : kSTK) stats_call(s[0], s[1], s[2], 0.25f, kGood);
    for (float min_conf : {0.f, -1.f, NAN, (float)INFINITY}) stats_call(2, 300, 17, min_conf, kGood);
    each_null(3, [](const Ptrs& P) { stats_call(2, 300, 17, 0.25f, P); });          // conf (1) may be null
    stats_call(0, 300, 17, 0.25f, null_at(2));          // null stats, bad shape

    for (auto& s : kSTK) hist_call(s[0], s[1], s[2], 32, 24, kGood);
    static const int kBins[][2] = {{1, 1},     {128, 128}, {128, 129}, {129, 128}, {16384, 1},  {1, 16385},      {0, 24},
                                   {32, 0},    {-1, 24},   {32, -1},   {kBig, kBig}, {kMax, kMax}, {65536, 65536}};
    for (auto& b : kBins) hist_call(2, 300, 17, b[0], b[1], kGood);
    each_null(5, [](const Ptrs& P) { hist_call(2, 300, 17, 32, 24, P); });          // conf (1) may be null
    hist_call(0, 300, 17, 32, 24, null_at(4));          // null counts, bad shape
    hist_call(65536, 300, 32768, 0, 24, kGood);         // bad shape, bad bin counts
    hist_call(2, 300, 17, 0, 16385, kGood);             // bad bin counts (0 x n is within the limit)
    hist_call(2, 300, 17, -1, -16385, kGood);           // bad bin counts, product beyond the limit
}

// ---- pk_spectrum.hip: grid (S K, ceil(F / 64)), then one workgroup per (sequence, joint)
static void spectrum_call(int S, int T, int K, int N, int j0, int F, int window, const Ptrs& P) {
    emit("motion_spectrum S=%d T=%d K=%d N=%d j0=%d F=%d window=%d", S, T, K, N, j0, F, window);
    tag(P);
    done(pk_motion_spectrum(P.f<float>(0), P.f<float>(1), P.f<double>(2), P.f<double>(3), S, T, K, 0.25f, N, j0, F, window, STREAM));
}
static void sweep_spectrum() {
    for (auto& s : kSTK) spectrum_call(s[0], s[1], s[2], 1024, 1, 64, 1, kGood);
    for (int F : {1, 63, 64, 65, 128, 129, 16384, 16385, 0, -1, kMax}) spectrum_call(2, 300, 17, 1 << 20, 1, F, 1, kGood);
    // the band against N / 2
    static const int kBand[][3] = {{256, 1, 128},  {256, 1, 129}, {256, 65, 64},    {256, 66, 64},          {256, 128, 1},       {256, 129, 1},
                                   {257, 1, 128},  {257, 1, 129}, {2, 1, 1},        {2, 1, 2},              {2, 2, 1},           {3, 1, 1},
                                   {3, 2, 1},      {1, 1, 1},     {0, 1, 1},        {-2, 1, 1},             {1 << 30, 1, 64},    {1 << 30, (1 << 29) - 63, 64},
                                   {1 << 30, (1 << 29) - 62, 64}, {(1 << 30) + 1, 1, 64}, {kMax, 1, 64},    {1 << 30, kMax, 64}, {1 << 20, kMax, 16384}};
    for (auto& b : kBand) spectrum_call(2, 300, 17, b[0], b[1], b[2], 0, kGood);
    for (int j0 : {0, -1, 1, 2}) spectrum_call(2, 300, 17, 1024, j0, 64, 0, kGood);
    for (int window : {0, 1, 2, -1}) spectrum_call(2, 300, 17, 1024, 1, 64, window, kGood);
    each_null(4, [](const Ptrs& P) { spectrum_call(2, 300, 17, 1024, 1, 64, 1, P); });          // conf (1) may be null
    spectrum_call(0, 300, 17, 1024, 1, 64, 1, null_at(3));       // two faults at once: null summary, bad shape
    spectrum_call(2, 0, 17, 1024, 1, 64, 2, kGood);              // bad shape, bad window
    spectrum_call(2, 300, 17, 1, 1, 64, 2, kGood);               // bad window, bad transform length
    spectrum_call(2, 300, 17, (1 << 30) + 1, 1, 16385, 0, kGood);          // bad transform length, too many bins
    spectrum_call(2, 300, 17, 1024, 0, 0, 0, kGood);             // no bins, bad first bin
    spectrum_call(2, 300, 17, 1024, 0, 513, 0, kGood);           // bad first bin (the band itself ends at N / 2)
    spectrum_call(2, 300, 17, 1024, 0, 514, 0, kGood);           // bad first bin, band beyond N / 2
}

// ---- pk_nms.hip: one lane per pose, one workgroup per image
static void rescore_call(int N, int K, double in_vis_thr, const Ptrs& P) {
    emit("pose_rescore N=%d K=%d in_vis_thr=%a", N, K, in_vis_thr);
    tag(P);
    done(pk_pose_rescore(P.f<double>(0), P.f<double>(1), P.f<double>(2), N, K, in_vis_thr, STREAM));
}
static void oks_nms_call(int n_img, int K, double thr, double in_vis_thr, int soft, int max_dets, const Ptrs& P) {
    emit("oks_nms n_img=%d K=%d thr=%a in_vis_thr=%a soft=%d max_dets=%d", n_img, K, thr, in_vis_thr, soft, max_dets);
    tag(P);
    done(pk_oks_nms(P.f<double>(0), P.f<double>(1), P.f<double>(2), P.f<int32_t>(3), P.f<double>(4), P.f<uint8_t>(5), P.f<int32_t>(6), P.f<int32_t>(7),
                    P.f<double>(8), n_img, K, thr, in_vis_thr, soft, max_dets, STREAM));
}
static const int kJoints[] = {1, 17, 34, 64, 65, 0, -1, kMax};
static void sweep_nms() {
    for (int N : {1, 255, 256, 257, kMax - 255, 0, -1}) rescore_call(N, 17, 0.2, kGood);
    for (int K : kJoints) rescore_call(257, K, 0.2, kGood);
    for (double v : {0.0, -1.0, (double)INFINITY, -(double)INFINITY, (double)NAN}) rescore_call(257, 17, v, kGood);
    each_null(3, [](const Ptrs& P) { rescore_call(257, 17, 0.2, P); });          // box_score (1) may be null
    rescore_call(0, 17, 0.2, null_at(0));               // two faults at once: null keypoints, bad size
    rescore_call(257, 65, (double)NAN, kGood);          // bad size, NaN threshold

    for (int n_img : {1, 34, 65535, 65536, kMax, 0, -1}) oks_nms_call(n_img, 17, 0.9, 0.2, 0, 20, kGood);
    for (int K : kJoints) oks_nms_call(34, K, 0.9, 0.2, 0, 20, kGood);
    for (int soft : {0, 1, 2, -1})
        for (double thr : {0.9, 0.0, -0.5, 1e-300, (double)INFINITY, -(double)INFINITY, (double)NAN})
            for (int max_dets : {20, 1, 0, -1}) oks_nms_call(34, 17, thr, 0.2, soft, max_dets, kGood);
    for (double v : {0.0, (double)INFINITY, -(double)INFINITY, (double)NAN}) oks_nms_call(34, 17, 0.9, v, 0, 20, kGood);
    each_null(9, [](const Ptrs& P) { oks_nms_call(34, 17, 0.9, 0.2, 0, 20, P); });
    oks_nms_call(0, 17, 0.9, 0.2, 0, 20, null_at(8));               // two faults at once: null out_score, bad size
    oks_nms_call(34, 65, (double)NAN, 0.2, 0, 20, kGood);           // bad size, NaN thr
    oks_nms_call(34, 17, (double)NAN, (double)NAN, 1, 0, kGood);    // NaN thresholds, soft mode without max_dets
    oks_nms_call(34, 17, 0.0, (double)NAN, 1, 0, kGood);            // NaN in_vis_thr, soft mode with thr = 0 and max_dets = 0
}

// ---- pk_eval.hip: COCO AP
static void coco_oks_call(int n_img, int K, int max_dets, const Ptrs& P) {
    emit("coco_kpt_oks n_img=%d K=%d max_dets=%d", n_img, K, max_dets);
    tag(P);
    done(pk_coco_kpt_oks(P.f<double>(0), P.f<double>(1), P.f<double>(2), P.f<int32_t>(3), P.f<double>(4), P.f<double>(5), P.f<int32_t>(6), P.f<double>(7),
                         P.f<int32_t>(8), P.f<int64_t>(9), P.f<int32_t>(10), P.f<double>(11), n_img, K, max_dets, STREAM));
}
static void coco_ws_call(int n_gt, int n_cap, int A, int T) {
    emit("coco_kpt_eval_ws_floats n_gt=%d n_cap=%d A=%d T=%d floats=%d", n_gt, n_cap, A, T, pk_coco_kpt_eval_ws_floats(n_gt, n_cap, A, T));
    done(PK_OK);
}
static void coco_eval_call(int n_img, int n_gt, int n_cap, int A, int T, int R, const Ptrs& P) {
    emit("coco_kpt_eval n_img=%d n_gt=%d n_cap=%d A=%d T=%d R=%d", n_img, n_gt, n_cap, A, T, R);
    tag(P);
    done(pk_coco_kpt_eval(P.f<double>(0), P.f<int64_t>(1), P.f<int32_t>(2), P.f<double>(3), P.f<int32_t>(4), P.f<int32_t>(5), P.f<int32_t>(6), P.f<double>(7),
                          P.f<double>(8), P.f<double>(9), P.f<double>(10), P.f<double>(11), P.f<int32_t>(12), P.f<uint8_t>(13), P.f<int32_t>(14),
                          P.f<int32_t>(15), P(16), P.f<double>(17), P.f<double>(18), n_img, n_gt, n_cap, A, T, R, STREAM));
}
static void sweep_eval() {
    for (int n_img : {1, 34, 65535, 65536, kMax, 0, -1}) coco_oks_call(n_img, 17, 20, kGood);
    for (int K : kJoints) coco_oks_call(34, K, 20, kGood);
    for (int max_dets : {1, 20, 64, 65, 0, -1, kMax}) coco_oks_call(34, 17, max_dets, kGood);
    each_null(12, [](const Ptrs& P) { coco_oks_call(34, 17, 20, P); });
    coco_oks_call(0, 17, 20, null_at(11));          // two faults at once: null oks, bad size
    coco_oks_call(34, 0, 65, kGood);                // bad size, more detections than the kernel is built for
    coco_oks_call(34, 65, 65, kGood);               // both limits

    // the (pr f64, tp i32) rows and the flag bytes of the overflow; the last ones leave 32 bits: the query does not refuse them
    static const int kWs[][4] = {{1, 1, 1, 1},       {7, 1, 1, 1},      {8, 1, 1, 1},       {9, 1, 1, 1},     {100, 257, 4, 10}, {6352, 10000, 4, 10},
                                 {0, 0, 4, 10},      {100, 257, 0, 0},  {-1, 257, 4, 10},   {100, -1, 4, 10}, {100, 257, -1, 10}, {100, 257, 4, -1},
                                 {1 << 20, 1 << 20, 8, 8}, {kMax, kMax, 8, 8}, {1 << 24, 11184810, 8, 8}, {1 << 24, 11184811, 8, 8}};
    for (auto& w : kWs) coco_ws_call(w[0], w[1], w[2], w[3]);

    for (int n_img : {1, 34, 65535, 65536, 0, -1}) coco_eval_call(n_img, 100, 257, 4, 10, 101, kGood);
    for (int n_gt : {1, 512, 513, 0, -1}) coco_eval_call(34, n_gt, 257, 4, 10, 101, kGood);
    for (int n_cap : {1, 255, 256, 257, 4096, 4097, kMax - 255, 0, -1}) coco_eval_call(34, 100, n_cap, 4, 10, 101, kGood);
    static const int kAT[][2] = {{1, 1}, {4, 10}, {8, 8}, {64, 1}, {1, 64}, {5, 13}, {65, 1}, {1, 65}, {0, 10}, {4, 0}, {-1, 10}, {4, -1}, {-8, -8}};
    for (auto& at : kAT) coco_eval_call(34, 100, 257, at[0], at[1], 101, kGood);
    for (int R : {1, 101, 0, -1}) coco_eval_call(34, 100, 257, 4, 10, R, kGood);
    each_null(19, [](const Ptrs& P) { coco_eval_call(34, 100, 257, 4, 10, 101, P); });
    coco_eval_call(34, 0, 257, 4, 10, 101, null_at(16));          // two faults at once: null workspace, bad size
    coco_eval_call(34, 100, 257, 65, 1, 0, kGood);                // bad size, too many curves
}

// ---- pk_draw.hip: shapes
struct ShapeCase {
    int N = 2, H = 480, W = 640, P = 3, K = 17, L = 19, C = 17, Q = 2, c0 = 0, c1 = 255, c2 = 0, box_thickness = 2, point_radius = 4, line_thickness = 2;
    float thr = 0.3f;
};
static void shapes_call(const ShapeCase& c, const Ptrs& P) {
    emit("draw_shapes N=%d H=%d W=%d P=%d K=%d L=%d C=%d Q=%d box=%d,%d,%d/%d thr=%a r=%d t=%d", c.N, c.H, c.W, c.P, c.K, c.L, c.C, c.Q, c.c0, c.c1, c.c2,
         c.box_thickness, (double)c.thr, c.point_radius, c.line_thickness);
    tag(P);
    done(pk_draw_shapes(P(0), c.N, c.H, c.W, P.f<float>(1), P.f<float>(2), P.f<int32_t>(3), c.P, c.K, P.f<int32_t>(4), c.L, P(5), c.C, P.f<float>(6),
                        P.f<int32_t>(7), c.Q, c.c0, c.c1, c.c2, c.box_thickness, c.thr, c.point_radius, c.line_thickness, STREAM));
}
template <class Set> static void shapes_with(Set set, const Ptrs& P = kGood) {
    ShapeCase c;
    set(c);
    shapes_call(c, P);
}
static void sweep_shapes() {
    shapes_call(ShapeCase{}, kGood);
    for (int N : {1, 65535, 65536, 0, -1}) shapes_with([N](ShapeCase& c) { c.N = N; });
    static const int kHW[][2] = {{1, 1}, {8, 32}, {9, 33}, {8, 31}, {7, 32}, {8192, 8192}, {8193, 8}, {8, 8193}, {0, 640}, {480, 0}, {-1, 640}, {480, -1}};
    for (auto& hw : kHW) shapes_with([&hw](ShapeCase& c) { c.H = hw[0], c.W = hw[1]; });
    for (int P : {1, 0, -1}) shapes_with([P](ShapeCase& c) { c.P = P; });
    for (int Q : {1, 0, -1}) shapes_with([Q](ShapeCase& c) { c.Q = Q; });
    for (int K : {1, 34, 0, -1}) shapes_with([K](ShapeCase& c) { c.K = K; });
    for (int L : {1, 0, -1}) shapes_with([L](ShapeCase& c) { c.L = L; });
    for (int C : {1, 0, -1}) shapes_with([C](ShapeCase& c) { c.C = C; });
    for (int r : {0, 1, 64, 65, -1}) shapes_with([r](ShapeCase& c) { c.point_radius = r; });
    for (int t : {1, 64, 65, 0, -1}) shapes_with([t](ShapeCase& c) { c.line_thickness = t; });
    for (int t : {1, 64, 65, 0, -1}) shapes_with([t](ShapeCase& c) { c.box_thickness = t; });
    for (int v : {0, 255, 256, -1}) {
        shapes_with([v](ShapeCase& c) { c.c0 = v; });
        shapes_with([v](ShapeCase& c) { c.c2 = v; });
    }
    for (float thr : {0.f, -1.f, NAN, (float)INFINITY}) shapes_with([thr](ShapeCase& c) { c.thr = thr; });
    // nothing to draw: no launch; only poses, only boxes: the other side's pointers and sizes are not looked at
    shapes_with([](ShapeCase& c) { c.P = 0, c.Q = 0; });
    shapes_with([](ShapeCase& c) { c.P = 0, c.Q = 0, c.K = 0, c.C = 0, c.box_thickness = 0, c.c0 = 256; });
    shapes_with([](ShapeCase& c) { c.Q = 0, c.box_thickness = 0, c.c0 = 256; });
    shapes_with([](ShapeCase& c) { c.P = 0, c.K = 0, c.C = 0, c.L = 5; });
    // P (L + K) + Q against 2^30
    shapes_with([](ShapeCase& c) { c.P = 1 << 20, c.L = 1000, c.K = 24, c.Q = 0; });
    shapes_with([](ShapeCase& c) { c.P = 1 << 20, c.L = 1000, c.K = 23, c.Q = (1 << 20) - 1; });
    shapes_with([](ShapeCase& c) { c.P = 1 << 20, c.L = 1000, c.K = 23, c.Q = 1 << 20; });
    shapes_with([](ShapeCase& c) { c.P = kMax, c.L = 1, c.K = 1, c.Q = kMax; });
    shapes_with([](ShapeCase& c) { c.P = 0, c.Q = (1 << 30) - 1; });
    shapes_with([](ShapeCase& c) { c.P = 0, c.Q = 1 << 30; });
    each_null(8, [](const Ptrs& P) { shapes_call(ShapeCase{}, P); });
    each_null(8, [](const Ptrs& P) { shapes_with([](ShapeCase& c) { c.P = 0; }, P); });
    each_null(8, [](const Ptrs& P) { shapes_with([](ShapeCase& c) { c.Q = 0; }, P); });
    shapes_with([](ShapeCase& c) { c.L = 0; }, null_at(4));                        // no limbs: no table needed
    shapes_with([](ShapeCase& c) { c.N = 0; }, null_at(0));                        // two faults at once: null image, bad batch shape
    shapes_with([](ShapeCase& c) { c.N = 65536, c.H = 8193; });                    // bad batch shape, image too large
    shapes_with([](ShapeCase& c) { c.W = 8193, c.P = -1; });                       // image too large, negative count
    shapes_with([](ShapeCase& c) { c.Q = -1, c.point_radius = 65; });              // negative count, bad radius
    shapes_with([](ShapeCase& c) { c.line_thickness = 0; }, null_at(1));           // bad thickness, null poses
    shapes_with([](ShapeCase& c) { c.K = 0; }, null_at(5));                        // null colours, bad pose tables
    shapes_with([](ShapeCase& c) { c.C = 0; }, null_at(6));                        // bad pose tables, null boxes
    shapes_with([](ShapeCase& c) { c.box_thickness = 65; }, null_at(7));           // null box index, bad box thickness
    shapes_with([](ShapeCase& c) { c.box_thickness = 0, c.c1 = 256; });            // bad box thickness, bad box colour
    shapes_with([](ShapeCase& c) { c.c1 = 256, c.P = 1 << 20, c.L = 1000, c.K = 24; });          // bad box colour, too many shapes
}

// ---- pk_draw.hip: heatmap overlays
struct OverlayCase {
    int N = 2, P = 5, K = 17, h = 64, w = 48, H = 256, W = 192;
    float alpha = 0.4f;
};
static void overlay_call(const OverlayCase& c, const Ptrs& P) {
    emit("heatmap_overlay N=%d K=%d h=%d w=%d H=%d W=%d alpha=%a ws_floats=%d", c.N, c.K, c.h, c.w, c.H, c.W, (double)c.alpha,
         pk_heatmap_overlay_ws_floats(c.N, c.K, c.h, c.w, c.H, c.W));
    tag(P);
    done(pk_heatmap_overlay(P(0), P.f<float>(1), c.alpha, P(2), P(3), P.f<float>(4), c.N, c.K, c.h, c.w, c.H, c.W, STREAM));
}
static void patches_call(const OverlayCase& c, const Ptrs& P) {
    emit("heatmap_overlay_patches N=%d P=%d K=%d h=%d w=%d H=%d W=%d alpha=%a ws_floats=%d", c.N, c.P, c.K, c.h, c.w, c.H, c.W, (double)c.alpha,
         pk_heatmap_overlay_patches_ws_floats(c.P, c.K, c.h, c.w));
    tag(P);
    done(pk_heatmap_overlay_patches(P(0), P.f<float>(1), P.f<int32_t>(2), P.f<double>(3), c.alpha, P(4), P(5), P(6), P.f<float>(7), c.N, c.P, c.K, c.h, c.w,
                                    c.H, c.W, STREAM));
}
template <class Call, class Set> static void overlay_with(Call call, Set set, const Ptrs& P = kGood) {
    OverlayCase c;
    set(c);
    call(c, P);
}
// what both overlay entries share: the batch, the joints, the planes against 8192, alpha
template <class Call> static void sweep_overlay_common(Call call) {
    call(OverlayCase{}, kGood);
    for (int N : {1, 65535, 65536, 0, -1}) overlay_with(call, [N](OverlayCase& c) { c.N = N, c.h = 4, c.w = 4; });
    for (int K : {1, 34, 0, -1}) overlay_with(call, [K](OverlayCase& c) { c.K = K; });
    static const int kPlane[][2] = {{1, 1}, {1, 255}, {1, 256}, {1, 257}, {8192, 8}, {8, 8192}, {8193, 8}, {8, 8193}, {0, 48}, {64, 0}, {-1, 48}, {64, -1}};
    for (auto& p : kPlane) overlay_with(call, [&p](OverlayCase& c) { c.h = p[0], c.w = p[1]; });
    // output planes of 1, 2047, 2048 and 2049 pixels, of 1023 / 1024 / 1025 pixels, tiles of 32 x 8, and on each side of 256 x 2048 pixels
    static const int kOut[][2] = {{1, 1},      {1, 2047},  {1, 2048},   {1, 2049},   {32, 64},    {1, 1023},  {1, 1024}, {1, 1025}, {8, 32},   {9, 33},
                                  {510, 1024}, {511, 1024}, {512, 1024}, {512, 1025}, {513, 1024}, {8192, 8192}, {8193, 8}, {8, 8193}, {0, 192}, {256, 0},
                                  {-1, 192},   {256, -1}};
    for (auto& o : kOut) overlay_with(call, [&o](OverlayCase& c) { c.H = o[0], c.W = o[1]; });
    for (float alpha : {0.f, 1.f, 2.f, -1.f, 0.001953125f, 0.005859375f, (float)INFINITY, NAN}) overlay_with(call, [alpha](OverlayCase& c) { c.alpha = alpha; });
}
static void sweep_overlays() {
    sweep_overlay_common(overlay_call);
    // N h w + 2 N ov_blocks against 2^31 - 1 floats
    overlay_with(overlay_call, [](OverlayCase& c) { c.N = 32, c.h = 8192, c.w = 8191, c.H = 8, c.W = 8; });
    overlay_with(overlay_call, [](OverlayCase& c) { c.N = 32, c.h = 8192, c.w = 8192, c.H = 8, c.W = 8; });
    overlay_with(overlay_call, [](OverlayCase& c) { c.N = 65535, c.h = 8192, c.w = 8192, c.H = 8192, c.W = 8192; });
    each_null(5, [](const Ptrs& P) { overlay_call(OverlayCase{}, P); });          // the index plane (3) may be null
    overlay_with(overlay_call, [](OverlayCase& c) { c.N = 0; }, null_at(4));                               // two faults at once: null workspace, bad shape
    overlay_with(overlay_call, [](OverlayCase& c) { c.K = 0, c.H = 8193; });                               // bad shape, plane too large
    overlay_with(overlay_call, [](OverlayCase& c) { c.N = 65535, c.h = 8193, c.w = 8192; });               // plane too large, workspace overflows
    overlay_with(overlay_call, [](OverlayCase& c) { c.N = 32, c.h = 8192, c.w = 8192, c.alpha = NAN; });   // workspace overflows, NaN alpha

    sweep_overlay_common(patches_call);
    for (int P : {1, 255, 256, 257, 65535, 65536, 0, -1}) overlay_with(patches_call, [P](OverlayCase& c) { c.P = P, c.h = 4, c.w = 4; });
    // P h w + 2 P against 2^31 - 1 floats
    overlay_with(patches_call, [](OverlayCase& c) { c.P = 32, c.h = 8192, c.w = 8191; });
    overlay_with(patches_call, [](OverlayCase& c) { c.P = 32, c.h = 8192, c.w = 8192; });
    overlay_with(patches_call, [](OverlayCase& c) { c.P = 65535, c.h = 181, c.w = 181; });
    overlay_with(patches_call, [](OverlayCase& c) { c.P = 65535, c.h = 182, c.w = 181; });
    each_null(8, [](const Ptrs& P) { patches_call(OverlayCase{}, P); });          // the index (5) and cover (6) planes may be null
    overlay_with(patches_call, [](OverlayCase& c) { c.P = 0; }, null_at(7));                                // two faults at once: null workspace, bad shape
    overlay_with(patches_call, [](OverlayCase& c) { c.N = 65536, c.P = 65536; });                           // bad shape, too many patches
    overlay_with(patches_call, [](OverlayCase& c) { c.P = 65536, c.H = 8193; });                            // too many patches, plane too large
    overlay_with(patches_call, [](OverlayCase& c) { c.P = 65535, c.h = 8193, c.w = 8192; });                // plane too large, workspace overflows
    overlay_with(patches_call, [](OverlayCase& c) { c.P = 32, c.h = 8192, c.w = 8192, c.alpha = NAN; });    // workspace overflows, NaN alpha
}

int main() {
    sweep_motion();
    sweep_spectrum();
    sweep_nms();
    sweep_eval();
    sweep_shapes();
    sweep_overlays();
    return 0;
}
