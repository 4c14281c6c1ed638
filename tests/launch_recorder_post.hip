// Host-only launch recorder for the library status, target, decode and input units and the entries that moved out of their common
// ancestor (tests/test_launch_routes_post.py): every extern "C" entry of pk_status.hip, pk_target.hip, pk_decode.hip and pk_input.hip,
// pk_rows_by_map / pk_drop_path_f32 of pk_layout.hip, pk_temporal_smooth / pk_nms_pose of pk_motion.hip and pk_pose_records of
// pk_eval.hip, swept over the smallest values at which each launch rule or argument check can go wrong.  One line per call: the problem,
// every launch (kernel, grid, block, LDS bytes, every argument: pointers as the made-up addresses, floats as hex floats, the 31 taps of
// k_unbiased_decode's and the 8 inverse scales of k_multiscale_merge's argument struct), the return code, the error text as
// pk_last_error_string gives it back (the library's own error state is compiled in), and the workspace query of the jittered crop.
//
// Build: hipcc --offload-host-only -O1 -std=c++17 -w tests/launch_recorder_post.hip -o launch_recorder_post
// -DPK_POST_SINGLE_UNIT='"/path/to/pk_target_decode.hip"' (with -I <csrc>) records from the single unit all of these were split from.
#define REC_LIBRARY_ERRORS
#include "launch_recorder.h"

#include <math.h>

#include <type_traits>

#ifdef PK_POST_SINGLE_UNIT
#include PK_POST_SINGLE_UNIT
#else
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_status.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_target.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_decode.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_input.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_layout.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_motion.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_eval.hip"
#endif

// ---- argument printers
static void rec_struct(const UbTaps& t) {
    emit(" {");
    for (int i = 0; i < UB_MAX_K; ++i) emit("%s%a", i ? " " : "", (double)t.v[i]);
    emit("}");
}
static void rec_struct(const MsInv& s) {
    emit(" {");
    for (int i = 0; i < 8; ++i) emit("%s%a", i ? " " : "", (double)s.v[i]);
    emit("}");
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

// ---- made-up addresses, one region per argument position; `null_at` knocks one pointer out, `mis_at` moves one `mis` bytes off its
// 16-byte alignment (0-based, -1: none).  Tables the entry itself reads on the host (filter taps, inverse scales, mean / std) are real.
struct Ptrs {
    int null_at, mis_at, mis;
    void* operator()(int k) const { return k == null_at ? nullptr : fake<void>(0x10000000u + 0x08000000u * (uintptr_t)k, k == mis_at ? mis : 0); }
    template <class T> T* f(int k) const { return (T*)(*this)(k); }
    const float* host(int k, const float* table) const { return k == null_at ? nullptr : table; }
};
static const Ptrs kGood{-1, -1, 0};
static Ptrs null_at(int k) { return Ptrs{k, -1, 0}; }
template <class Call> static void each_null(int n, Call call) {
    for (int k = 0; k < n; ++k) call(null_at(k));
}
static void tag(const Ptrs& P) { emit(" null=%d mis=%d+%d", P.null_at, P.mis_at, P.mis); }
static void done(int rc) {
    finish(rc);
    flush_line();
}
static const int kBig = 46341;          // kBig * kBig is the first square above 2^31

// ---- library status
static void sweep_status() {
    emit("status version=%d error=\"%s\"", pk_version(), pk_last_error_string());
    flush_line();
    for (int id : {0, 1, 65535, 65536, -1}) {
        emit("marker id=%d", id);
        done(pk_marker(id, STREAM));
    }
}

// ---- T1 / T2
static void gauss_call(int B, int K, int H, int W, int lut_len, double sx, double sy, double reach, int pn, int pc, const Ptrs& P) {
    emit("gaussian_target B=%d K=%d H=%d W=%d lut=%d sx=%a sy=%a reach=%a pn=%d pc=%d", B, K, H, W, lut_len, sx, sy, reach, pn, pc);
    tag(P);
    done(pk_gaussian_target(P.f<float>(0), P.f<float>(1), P.f<float>(2), lut_len, P.f<float>(3), P.f<float>(4), B, K, H, W, sx, sy, reach, pn, pc, STREAM));
}
static void dense_call(int B, int K, int H, int W, float sigma, const Ptrs& P) {
    emit("dense_target B=%d K=%d H=%d W=%d sigma=%a", B, K, H, W, (double)sigma);
    tag(P);
    done(pk_dense_target(P.f<float>(0), P.f<float>(1), P.f<float>(2), P.f<float>(3), B, K, H, W, 0.25f, 0.25f, sigma, STREAM));
}
static void sweep_target() {
    // a 13-wide patch centred at 6 reaches 6 pixels and needs 2 * 6 * 6 + 1 = 73 table entries
    static const int kBK[][2] = {{1, 1}, {2, 17}, {0, 17}, {2, 0}, {-1, 17}};
    for (auto& bk : kBK) gauss_call(bk[0], bk[1], 64, 48, 73, 4.0, 4.0, 6.0, 13, 6, kGood);
    static const int kHW[][2] = {{7, 5}, {1, 1}, {0, 48}, {64, 0}, {64, -1}, {kBig, kBig}};
    for (auto& hw : kHW) gauss_call(2, 17, hw[0], hw[1], 73, 4.0, 4.0, 6.0, 13, 6, kGood);
    for (int lut : {72, 73, 74, 0}) gauss_call(2, 17, 64, 48, lut, 4.0, 4.0, 6.0, 13, 6, kGood);
    for (int lut : {200, 201}) gauss_call(2, 17, 64, 48, lut, 4.0, 4.0, 2.0, 13, 2, kGood);          // off-centre: the far side counts
    for (int lut : {200, 201}) gauss_call(2, 17, 64, 48, lut, 4.0, 4.0, 2.0, 13, 10, kGood);
    for (double reach : {6.0, 6.25, 6.5, 7.0, 0.0, -1.0, 0.25}) gauss_call(2, 17, 64, 48, 73, 4.0, 4.0, reach, 13, 6, kGood);
    for (int pc : {-1, 0, 12, 13}) gauss_call(2, 17, 64, 48, 289, 4.0, 4.0, 6.0, 13, pc, kGood);
    for (int pn : {0, -1, 1, 12}) gauss_call(2, 17, 64, 48, 289, 4.0, 4.0, 0.5, pn, 0, kGood);
    static const double kStride[][2] = {{0.0, 4.0}, {4.0, 0.0}, {-4.0, 4.0}, {4.0, NAN}, {1e-300, 1e300}};
    for (auto& s : kStride) gauss_call(2, 17, 64, 48, 73, s[0], s[1], 6.0, 13, 6, kGood);
    each_null(5, [](const Ptrs& P) { gauss_call(2, 17, 64, 48, 73, 4.0, 4.0, 6.0, 13, 6, P); });
    for (int off : {4, 8, 12}) gauss_call(2, 17, 64, 48, 73, 4.0, 4.0, 6.0, 13, 6, Ptrs{-1, 3, off});
    gauss_call(2, 17, 64, 48, 73, 4.0, 4.0, 6.0, 13, 6, Ptrs{-1, 2, 4});          // only the target has to be aligned
    // two faults at once: which check comes first
    gauss_call(0, 17, 64, 48, 73, 4.0, 4.0, 6.0, 13, 6, null_at(0));              // null, bad shape
    gauss_call(0, 17, 64, 48, 73, 0.0, 4.0, 6.0, 13, 6, kGood);                   // bad shape, bad stride
    gauss_call(2, 17, 64, 48, 72, 4.0, 4.0, 0.0, 13, 6, kGood);                   // bad reach, short table
    gauss_call(2, 17, 64, 48, 72, 4.0, 4.0, 7.0, 13, 6, kGood);                   // short table, reach beyond the patch
    gauss_call(2, 17, 64, 48, 73, 4.0, 4.0, 7.0, 13, 6, Ptrs{-1, 3, 4});          // reach beyond the patch, misaligned target

    for (auto& bk : kBK) dense_call(bk[0], bk[1], 64, 48, 2.f, kGood);
    for (auto& hw : kHW) dense_call(2, 17, hw[0], hw[1], 2.f, kGood);
    for (float sigma : {0.f, -1.f, NAN, 1e-30f}) dense_call(2, 17, 64, 48, sigma, kGood);
    each_null(4, [](const Ptrs& P) { dense_call(2, 17, 64, 48, 2.f, P); });
    dense_call(2, 17, 64, 48, 0.f, null_at(3));          // null, bad sigma
}

// ---- decoders: one workgroup per map
static const int kMaps[] = {1, 34, 0, -1};
static const int kMapHW[][2] = {{64, 48}, {7, 5}, {1, 1}, {0, 48}, {64, 0}, {-1, 48}, {46340, 46340}, {kBig, kBig}, {1, 0x7fffffff}, {2, 0x40000000}};
static void argmax_call(int BK, int H, int W, int mode, const Ptrs& P) {
    emit("argmax_decode BK=%d H=%d W=%d mode=%d", BK, H, W, mode);
    tag(P);
    done(pk_argmax_decode(P.f<float>(0), P.f<int32_t>(1), P.f<float>(2), P.f<float>(3), BK, H, W, mode, STREAM));
}
static void unbiased_call(int BK, int H, int W, int ksize, const Ptrs& P) {
    static float taps[33];
    for (int t = 0; t < 33; ++t) taps[t] = 1.f / (float)(t + 3);          // distinct: the zero fill beyond ksize shows
    emit("unbiased_decode BK=%d H=%d W=%d ksize=%d", BK, H, W, ksize);
    tag(P);
    done(pk_unbiased_decode(P.f<float>(0), P.host(1, taps), ksize, P.f<int32_t>(2), P.f<float>(3), P.f<float>(4), P.f<uint8_t>(5), BK, H, W, STREAM));
}
static void softargmax_call(int BK, int H, int W, int radius, const Ptrs& P) {
    emit("softargmax_refine_decode BK=%d H=%d W=%d radius=%d", BK, H, W, radius);
    tag(P);
    done(pk_softargmax_refine_decode(P.f<float>(0), P.f<float>(1), P.f<float>(2), P.f<float>(3), P.f<float>(4), P.f<float>(5), BK, H, W, radius, STREAM));
}
static void softargmax_bwd_call(int BK, int H, int W, const Ptrs& P) {
    emit("softargmax_bwd BK=%d H=%d W=%d", BK, H, W);
    tag(P);
    done(pk_softargmax_bwd(P.f<float>(0), P.f<float>(1), P.f<float>(2), P.f<float>(3), P.f<float>(4), P.f<float>(5), BK, H, W, STREAM));
}
static void flip_call(int B, int K, int H, int W, const Ptrs& P) {
    emit("flip_merge B=%d K=%d H=%d W=%d", B, K, H, W);
    tag(P);
    done(pk_flip_merge(P.f<float>(0), P.f<float>(1), P.f<int32_t>(2), P.f<float>(3), B, K, H, W, STREAM));
}
static void multiscale_call(int S, int F, int B, int K, int H, int W, const float* inv, const Ptrs& P) {
    emit("multiscale_merge S=%d F=%d B=%d K=%d H=%d W=%d inv=", S, F, B, K, H, W);
    for (int s = 0; s < 9; ++s) emit("%s%a", s ? "," : "", (double)inv[s]);
    tag(P);
    done(pk_multiscale_merge(P.f<float>(0), P.f<int32_t>(1), P.host(2, inv), P.f<float>(3), S, F, B, K, H, W, STREAM));
}
static void sweep_decode_maps() {
    for (int BK : kMaps) argmax_call(BK, 64, 48, 0, kGood);
    for (auto& hw : kMapHW) argmax_call(34, hw[0], hw[1], 0, kGood);
    for (int mode : {-1, 0, 1, 2, 3}) argmax_call(34, 64, 48, mode, kGood);
    each_null(4, [](const Ptrs& P) { argmax_call(34, 64, 48, 2, P); });
    argmax_call(0, 64, 48, 2, null_at(0));          // two faults at once: null heatmaps, bad shape
    argmax_call(34, kBig, kBig, 3, kGood);          // bad shape, bad mode

    for (int BK : kMaps) unbiased_call(BK, 64, 48, 11, kGood);
    for (auto& hw : kMapHW) unbiased_call(34, hw[0], hw[1], 11, kGood);
    for (int ksize : {1, 2, 3, 11, 31, 33, 0, -1, 5, 29, 30, 32}) unbiased_call(34, 64, 48, ksize, kGood);
    each_null(6, [](const Ptrs& P) { unbiased_call(34, 64, 48, 11, P); });
    unbiased_call(34, 64, 48, 2, null_at(4));             // two faults at once: null coords, even ksize
    unbiased_call(34, kBig, kBig, 33, kGood);             // ksize too large, bad shape

    for (int BK : kMaps) softargmax_call(BK, 64, 48, 2, kGood);
    for (auto& hw : kMapHW) softargmax_call(34, hw[0], hw[1], 2, kGood);
    for (int radius : {-1, 0, 1, 2, 100}) softargmax_call(34, 64, 48, radius, kGood);
    each_null(6, [](const Ptrs& P) { softargmax_call(34, 64, 48, 2, P); });
    softargmax_call(34, 64, 48, -1, null_at(3));          // two faults at once: offsets without fusion_weight, bad radius
    softargmax_call(0, 64, 48, 2, null_at(2));            // null alpha, bad shape

    for (int BK : kMaps) softargmax_bwd_call(BK, 64, 48, kGood);
    for (auto& hw : kMapHW) softargmax_bwd_call(34, hw[0], hw[1], kGood);
    each_null(6, [](const Ptrs& P) { softargmax_bwd_call(34, 64, 48, P); });

    static const int kBK[][2] = {{1, 1}, {2, 17}, {34, 1}, {0, 17}, {2, 0}, {-1, 17}};
    for (auto& bk : kBK) flip_call(bk[0], bk[1], 64, 48, kGood);
    for (auto& hw : kMapHW) flip_call(2, 17, hw[0], hw[1], kGood);
    each_null(4, [](const Ptrs& P) { flip_call(2, 17, 64, 48, P); });

    static const float inv[9] = {1.25f, 1.f, 0.8f, 2.f, 0.5f, 1.5f, 0.75f, 0.625f, 3.f};
    for (int S : {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1}) multiscale_call(S, 2, 2, 17, 64, 48, inv, kGood);
    for (int F : {0, 1, 2, 3}) multiscale_call(3, F, 2, 17, 64, 48, inv, kGood);
    for (int F : {2, 1}) multiscale_call(3, F, 2, 17, 64, 48, inv, null_at(1));
    for (auto& bk : kBK) multiscale_call(3, 2, bk[0], bk[1], 64, 48, inv, kGood);
    for (int K : {32767, 32768}) multiscale_call(3, 2, 65536, K, 64, 48, inv, kGood);          // B * K against 2^31
    for (auto& hw : kMapHW) multiscale_call(3, 2, 2, 17, hw[0], hw[1], inv, kGood);
    for (float bad : {0.f, -1.f, (float)INFINITY, NAN, 1e-45f}) {
        for (int at : {0, 2, 3}) {          // inside the S = 3 that are read, and beyond them
            float v[9];
            memcpy(v, inv, sizeof(v));
            v[at] = bad;
            multiscale_call(3, 2, 2, 17, 64, 48, v, kGood);
        }
    }
    each_null(4, [](const Ptrs& P) { multiscale_call(3, 2, 2, 17, 64, 48, inv, P); });
    multiscale_call(3, 3, 2, 17, 64, 48, inv, null_at(0));          // two faults at once: null stack, bad F
    multiscale_call(9, 3, 2, 17, 64, 48, inv, kGood);               // bad F, bad S
    multiscale_call(9, 2, 2, 17, 64, 48, inv, null_at(1));          // no partner table, bad S
    multiscale_call(9, 2, 0, 17, 64, 48, inv, kGood);               // bad S, bad shape
    {
        float v[9];
        memcpy(v, inv, sizeof(v));
        v[0] = 0.f;
        multiscale_call(3, 2, 2, 17, kBig, kBig, v, kGood);         // bad shape, bad inverse scale
    }
}

// ---- decoders and post-processing: one lane per map
static const int kLanes[] = {1, 255, 256, 257, 0, -1};
static void local_refine_call(int BK, int H, int W, int radius, const Ptrs& P) {
    emit("local_gaussian_refine BK=%d H=%d W=%d radius=%d", BK, H, W, radius);
    tag(P);
    done(pk_local_gaussian_refine(P.f<float>(0), P.f<float>(1), P.f<float>(2), BK, H, W, radius, STREAM));
}
static void window_refine_call(int BK, int H, int W, int window, const Ptrs& P) {
    emit("window_refine BK=%d H=%d W=%d window=%d", BK, H, W, window);
    tag(P);
    done(pk_window_refine(P.f<float>(0), P.f<float>(1), P.f<float>(2), BK, H, W, window, STREAM));
}
static void blend_call(int BK, const Ptrs& P) {
    emit("fused_blend BK=%d", BK);
    tag(P);
    done(pk_fused_blend(P.f<float>(0), P.f<float>(1), P.f<float>(2), P.f<float>(3), BK, 4.f, 4.f, 256.f, STREAM));
}
static void affine_coords_call(int B, int K, const Ptrs& P) {
    emit("affine_coords B=%d K=%d", B, K);
    tag(P);
    done(pk_affine_coords(P.f<float>(0), P.f<float>(1), P.f<float>(2), P.f<float>(3), B, K, 0.0625f, 0.0625f, P.f<float>(4), 0.2f, STREAM));
}
static void smooth_call(int T, int C, int window, const Ptrs& P) {
    emit("temporal_smooth T=%d C=%d window=%d", T, C, window);
    tag(P);
    done(pk_temporal_smooth(P.f<float>(0), P.f<float>(1), P.f<double>(2), T, C, window, STREAM));
}
static void nms_call(int B, int K, const Ptrs& P) {
    emit("nms_pose B=%d K=%d", B, K);
    tag(P);
    done(pk_nms_pose(P.f<float>(0), P.f<float>(1), P.f<float>(2), P.f<uint8_t>(3), B, K, 10.f, STREAM));
}
static void records_call(int B, int K, const Ptrs& P) {
    emit("pose_records B=%d K=%d", B, K);
    tag(P);
    done(pk_pose_records(P.f<float>(0), P.f<float>(1), P.f<float>(2), P.f<float>(3), B, K, STREAM));
}
static void sweep_lanes() {
    static const int kHW[][2] = {{64, 48}, {1, 1}, {0, 48}, {64, 0}, {kBig, kBig}};
    for (int n : kLanes) local_refine_call(n, 64, 48, 2, kGood);
    for (auto& hw : kHW) local_refine_call(34, hw[0], hw[1], 2, kGood);
    for (int radius : {-1, 0, 2}) local_refine_call(34, 64, 48, radius, kGood);
    each_null(3, [](const Ptrs& P) { local_refine_call(34, 64, 48, 2, P); });

    for (int n : kLanes) window_refine_call(n, 64, 48, 5, kGood);
    for (auto& hw : kHW) window_refine_call(34, hw[0], hw[1], 5, kGood);
    for (int window : {-1, 0, 1, 4, 5}) window_refine_call(34, 64, 48, window, kGood);
    each_null(3, [](const Ptrs& P) { window_refine_call(34, 64, 48, 5, P); });

    for (int n : kLanes) blend_call(n, kGood);
    each_null(4, [](const Ptrs& P) { blend_call(34, P); });
    blend_call(34, Ptrs{1, -1, 0});
    {
        Ptrs none{1, -1, 0};          // neither maxvals nor regression: the plain scaling
        emit("fused_blend BK=34 no regression");
        done(pk_fused_blend(none.f<float>(0), nullptr, nullptr, none.f<float>(3), 34, 4.f, 4.f, 256.f, STREAM));
    }

    static const int kBK[][2] = {{1, 1}, {15, 17}, {16, 16}, {1, 257}, {257, 1}, {0, 17}, {15, 0}, {-1, 17}};
    for (auto& bk : kBK) affine_coords_call(bk[0], bk[1], kGood);
    each_null(5, [](const Ptrs& P) { affine_coords_call(15, 17, P); });

    static const int kTC[][2] = {{1, 1}, {15, 17}, {8, 32}, {257, 1}, {1, 34}, {0, 34}, {100, 0}, {-1, 34}};
    for (auto& tc : kTC) smooth_call(tc[0], tc[1], 5, kGood);
    for (int window : {-1, 0, 1, 2, 4, 5}) smooth_call(100, 34, window, kGood);
    each_null(3, [](const Ptrs& P) { smooth_call(100, 34, 5, P); });
    smooth_call(0, 34, 4, kGood);                  // two faults at once: bad shape, even window
    smooth_call(100, 34, 4, null_at(2));           // null weights, even window

    for (int B : {1, 63, 64, 65, 0, -1}) nms_call(B, 17, kGood);
    for (int K : {1, 0, -1}) nms_call(65, K, kGood);
    each_null(4, [](const Ptrs& P) { nms_call(65, 17, P); });

    for (int B : {1, 34, 65, 0, -1}) records_call(B, 17, kGood);
    for (int K : {1, 64, 65, 0, -1}) records_call(34, K, kGood);
    each_null(4, [](const Ptrs& P) { records_call(34, 17, P); });
}

// ---- window partition / reverse and DropPath: grid-stride launches of at most 4096 workgroups
static void rows_call(int64_t n_rows, int row_bytes, int scatter, const Ptrs& P) {
    emit("rows_by_map n_rows=%lld row_bytes=%d scatter=%d", (long long)n_rows, row_bytes, scatter);
    tag(P);
    done(pk_rows_by_map(P(0), P(1), P.f<int>(2), n_rows, row_bytes, scatter, STREAM));
}
static void drop_call(int64_t batch, int64_t per_sample, float keep, const Ptrs& P) {
    emit("drop_path batch=%lld per_sample=%lld keep=%a", (long long)batch, (long long)per_sample, (double)keep);
    tag(P);
    done(pk_drop_path_f32(P.f<float>(0), P.f<float>(1), P.f<float>(2), batch, per_sample, keep, STREAM));
}
static void sweep_strided() {
    // totals on each side of a workgroup, of the 4096-workgroup cap, beyond 32 bits, and so large that the workgroup count itself is
    static const int64_t kTotal[] = {1, 255, 256, 257, 1048575, 1048576, 1048577, ((int64_t)1 << 32) + 1, (int64_t)1 << 41, ((int64_t)1 << 39) + 1};
    for (int scatter = 0; scatter < 2; ++scatter) {
        for (int64_t t : kTotal) rows_call(t, 4, scatter, kGood);
        for (int row_bytes : {0, 2, 4, 6, 8, 128, -4}) rows_call(257, row_bytes, scatter, kGood);
        for (int64_t rows : {(int64_t)131071, (int64_t)131072, (int64_t)131073}) rows_call(rows, 32, scatter, kGood);          // the cap through the row width
        for (int64_t rows : {(int64_t)0, (int64_t)-1}) rows_call(rows, 4, scatter, kGood);
    }
    rows_call(257, 128, 2, kGood);
    each_null(3, [](const Ptrs& P) { rows_call(257, 128, 0, P); });
    rows_call(0, 6, 0, null_at(0));

    for (int64_t t : kTotal) drop_call(1, t, 0.9f, kGood);
    for (int64_t t : kTotal) drop_call(t, 1, 0.9f, kGood);
    drop_call(34, 30841, 0.9f, kGood);
    drop_call(34, 30842, 0.9f, kGood);          // 34 * 30842 = 1 048 628: capped
    for (float keep : {0.f, -0.5f, NAN, 1e-30f, 1.f}) drop_call(34, 3072, keep, kGood);
    static const int64_t kBad[][2] = {{0, 3072}, {34, 0}, {-1, 3072}, {34, -1}};
    for (auto& b : kBad) drop_call(b[0], b[1], 0.9f, kGood);
    each_null(3, [](const Ptrs& P) { drop_call(34, 3072, 0.9f, P); });
    drop_call(0, 3072, 0.f, null_at(1));
}

// ---- the input pipeline
static const float kMean[3] = {0.485f, 0.456f, 0.406f}, kStd[3] = {0.229f, 0.224f, 0.225f};
static const int OUT_NCHW = 1, OUT_NHWC = 2;
static void crop_call(int n, int w, int h, int outs, const Ptrs& P) {
    emit("affine_crop_normalize n=%d w=%d h=%d outs=%d", n, w, h, outs);
    tag(P);
    done(pk_affine_crop_normalize(P(0), P(1), n, w, h, (outs & OUT_NCHW) ? P.f<float>(2) : nullptr, (outs & OUT_NHWC) ? P(3) : nullptr, P.host(4, kMean),
                                  P.host(5, kStd), STREAM));
}
// ws_delta: bytes added to the size the query asks for (0 where the query refuses the shape)
static void jitter_call(int n, int w, int h, int outs, int64_t ws_delta, const Ptrs& P) {
    const int need = pk_affine_crop_jitter_ws_bytes(n, w, h);
    emit("affine_crop_jitter_normalize n=%d w=%d h=%d outs=%d ws_bytes=%d", n, w, h, outs, need);
    if (need < 0) emit(" query_err=\"%s\"", pk_last_error_string());
    emit(" ws_delta=%lld", (long long)ws_delta);
    tag(P);
    done(pk_affine_crop_jitter_normalize(P(0), P(1), P(6), n, w, h, (outs & OUT_NCHW) ? P.f<float>(2) : nullptr, (outs & OUT_NHWC) ? P(3) : nullptr,
                                         P.host(4, kMean), P.host(5, kStd), P(7), (need > 0 ? need : 0) + ws_delta, STREAM));
}
static void sweep_input() {
    // planes of 255, 256 and 257 pixels, the two network inputs, 765 * 2370 * 2370 >= 2^32 > 765 * 2369 * 2369
    static const int kWH[][2] = {{15, 17}, {16, 16}, {257, 1}, {1, 1}, {192, 256}, {288, 384}, {2369, 2369}, {2370, 2370}, {0, 256}, {192, 0}, {-1, 256}};
    for (auto& wh : kWH) for (int outs : {OUT_NCHW, OUT_NHWC, OUT_NCHW | OUT_NHWC}) crop_call(3, wh[0], wh[1], outs, kGood);
    for (int n : {1, 64, 65535, 65536, 0, -1}) crop_call(n, 192, 256, OUT_NCHW | OUT_NHWC, kGood);
    crop_call(3, 192, 256, 0, kGood);
    each_null(6, [](const Ptrs& P) { crop_call(3, 192, 256, OUT_NCHW | OUT_NHWC, P); });
    for (int off : {2, 4, 8}) crop_call(3, 192, 256, OUT_NCHW | OUT_NHWC, Ptrs{-1, 3, off});
    crop_call(3, 192, 256, OUT_NCHW, Ptrs{-1, 3, 8});                      // an NHWC output that is not asked for
    crop_call(3, 192, 256, OUT_NCHW | OUT_NHWC, Ptrs{-1, 2, 8});           // only the NHWC output has to be aligned
    crop_call(0, 192, 256, OUT_NCHW | OUT_NHWC, Ptrs{-1, 3, 8});           // two faults at once: bad shape, misaligned NHWC output
    crop_call(3, 192, 256, OUT_NCHW | OUT_NHWC, Ptrs{4, 3, 8});            // null mean, misaligned NHWC output

    for (auto& wh : kWH) for (int outs : {OUT_NCHW, OUT_NHWC, OUT_NCHW | OUT_NHWC}) jitter_call(3, wh[0], wh[1], outs, 0, kGood);
    for (int n : {1, 64, 95, 96, 0, -1}) jitter_call(n, 2369, 2369, OUT_NCHW | OUT_NHWC, 0, kGood);          // the workspace against 2^31 bytes
    jitter_call(3, kBig, kBig, OUT_NCHW | OUT_NHWC, 0, kGood);
    jitter_call(3, 192, 256, 0, 0, kGood);
    for (int64_t delta : {(int64_t)-1, (int64_t)1, (int64_t)1 << 33}) jitter_call(3, 192, 256, OUT_NCHW | OUT_NHWC, delta, kGood);
    jitter_call(3, 192, 256, OUT_NCHW | OUT_NHWC, -((int64_t)1 << 40), kGood);
    each_null(8, [](const Ptrs& P) { jitter_call(3, 192, 256, OUT_NCHW | OUT_NHWC, 0, P); });
    for (int off : {1, 2, 4, 8}) jitter_call(3, 192, 256, OUT_NCHW | OUT_NHWC, 0, Ptrs{-1, 7, off});
    for (int off : {2, 4, 8}) jitter_call(3, 192, 256, OUT_NCHW | OUT_NHWC, 0, Ptrs{-1, 3, off});
    jitter_call(3, 192, 256, OUT_NCHW, 0, Ptrs{-1, 3, 8});
    jitter_call(3, 2370, 2370, OUT_NCHW | OUT_NHWC, 0, null_at(6));             // two faults at once: null jitter table, crop too large
    jitter_call(3, 2370, 2370, OUT_NCHW | OUT_NHWC, -1, Ptrs{-1, 7, 2});        // crop too large, workspace too small and misaligned
    jitter_call(3, 192, 256, OUT_NCHW | OUT_NHWC, -1, Ptrs{-1, 7, 2});          // workspace too small, misaligned
    jitter_call(3, 192, 256, OUT_NCHW | OUT_NHWC, 0, Ptrs{7, 3, 8});            // null workspace, misaligned NHWC output
    for (int n : {96, 95}) {
        emit("affine_crop_jitter_ws_bytes n=%d w=2369 h=2369", n);
        done(pk_affine_crop_jitter_ws_bytes(n, 2369, 2369) < 0 ? PK_ERR_INVALID : PK_OK);
    }
}

int main() {
    sweep_status();
    sweep_target();
    sweep_decode_maps();
    sweep_lanes();
    sweep_strided();
    sweep_input();
    return 0;
}
