// Host-only launch recorder for the fused block halves and the window-attention core (tests/test_launch_routes_block.py): every
// extern "C" entry of pk_block_mlp.hip, pk_block_attn.hip and pk_attn.hip, swept over the smallest values at which each launch rule can
// go wrong.  One line per call: the problem, every launch (kernel, grid, block, LDS bytes) with the launcher-set fields of its argument
// block (MlpArgs / AttnArgs: sizes, eps and softmax_scale as hex floats, a bit per non-null pointer field and the pointers themselves) and
// its trailing arguments, the return code, the error text and the size queries for the same problem.
//
// Build: hipcc --offload-host-only -O1 -std=c++17 tests/launch_recorder_block.hip -o launch_recorder_block
// -DPK_BLOCK_SINGLE_UNIT='"/path/to/pk_block.hip"' (with -I <csrc>) records from the single unit the two block units were split from.
#include "launch_recorder.h"

#include <type_traits>

#include "../infantposeestimation_gaussianbias_amd/csrc/pk_attn.hip"
#ifdef PK_BLOCK_SINGLE_UNIT
#include PK_BLOCK_SINGLE_UNIT
#else
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_block_mlp.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_block_attn.hip"
#endif

// ---- argument printers
static void rec_ptrs(const void* const* p, int n) {
    unsigned mask = 0;
    for (int i = 0; i < n; ++i) mask |= p[i] ? 1u << i : 0u;
    emit(" ptrs=%x", mask);
    for (int i = 0; i < n; ++i) emit(" %lx", (unsigned long)(uintptr_t)p[i]);
    emit("}");
}
static void rec_struct(const MlpArgs& a) {
    const void* const p[] = {a.x, a.dy, a.out, a.gamma, a.beta, a.b1, a.b2, a.scale, a.w1, a.w2, a.w1t, a.w2t, a.part};
    emit(" {M=%d rps=%d eps=%a", a.M, a.rows_per_sample, (double)a.eps);
    rec_ptrs(p, 13);
}
static void rec_struct(const AttnArgs& a) {
    const void* const p[] = {a.x, a.dy, a.out, a.rowmap, a.gamma, a.beta, a.table, a.bqkv, a.bproj, a.scale, a.wqkv, a.wproj, a.wqkv_t, a.wproj_t,
                             a.o_save, a.lse, a.dqkv, a.u_save, a.part};
    emit(" {nw=%d wps=%d eps=%a ss=%a", a.n_windows, a.windows_per_sample, (double)a.eps, (double)a.softmax_scale);
    rec_ptrs(p, 19);
}
template <class T> static void rec_val(const T& v) {
    if constexpr (std::is_pointer_v<T>) emit(" %lx", (unsigned long)(uintptr_t)v);
    else if constexpr (std::is_floating_point_v<T>) emit(" %a", (double)v);
    else if constexpr (std::is_integral_v<T>) emit(" %lld", (long long)v);
    else rec_struct(v);
}
// the argument block alone (k_mlp_fwd, k_attn_fwd, ...), with trailing scalars (k_mlp_fwd_w: C, c_real, HD; k_attn_fwd_w: C, c_real) or
// pointers (k_attn_bwd: the two slab arrays), and the plain argument lists of pk_attn.hip's kernels
template <class... A> static void rec_args(Rec, const A&... a) {
    emit(" a=");
    (rec_val(a), ...);
}

// ---- made-up addresses, one region per argument position; `null_at` knocks one pointer out, `mis_at` moves one 8 bytes off its
// 16-byte alignment (0-based, -1: none)
struct Ptrs {
    int null_at, mis_at;
    void* operator()(int k) const { return k == null_at ? nullptr : fake<void>(0x10000000u + 0x08000000u * (uintptr_t)k, k == mis_at ? 8 : 0); }
    template <class T> T* f(int k) const { return (T*)(*this)(k); }
};
static const Ptrs kGood{-1, -1};
// every pointer position of an entry: null, then misaligned
template <class Call> static void each_pointer(int n, Call call) {
    for (int k = 0; k < n; ++k) call(Ptrs{k, -1});
    for (int k = 0; k < n; ++k) call(Ptrs{-1, k});
}

// ---- fused MLP half, C = 32 / 64
enum { MLP_FWD, MLP_DX, MLP_DW };
static void mlp_call(int which, int M, int C, int rps, int sc, const Ptrs& P) {
    static const char* const name[] = {"mlp_fwd", "mlp_dx", "mlp_dw"};
    emit("%s M=%d C=%d rps=%d sc=%d null=%d mis=%d", name[which], M, C, rps, sc, P.null_at, P.mis_at);
    const float* scale = sc ? P.f<float>(9) : nullptr;
    if (which == MLP_FWD)
        finish(pk_ln_mlp_fwd(P(1), P.f<float>(2), P.f<float>(3), P(4), P.f<float>(5), P(6), P.f<float>(7), scale, P(8), M, C, rps, 1e-5f, STREAM));
    else if (which == MLP_DX)
        finish(pk_ln_mlp_bwd_dx(P(0), P(1), P.f<float>(2), P.f<float>(3), P(4), P.f<float>(5), P(10), P(11), scale, P(8), P.f<float>(12), M, C, rps, 1e-5f, STREAM));
    else
        finish(pk_ln_mlp_bwd_dw(P(0), P(1), P.f<float>(2), P.f<float>(3), P(4), P.f<float>(5), P(11), scale, P.f<float>(12), M, C, rps, 1e-5f, STREAM));
    emit(" dx_blocks=%d dw_blocks=%d", pk_ln_mlp_dx_blocks(M, C), pk_ln_mlp_dw_blocks(M, C));
    flush_line();
}
static void sweep_mlp() {
    for (int C : {32, 64, 48, 0}) {
        emit("mlp_queries C=%d supported=%d hidden_slice=%d slab_floats=%d", C, pk_ln_mlp_supported(C), pk_ln_mlp_hidden_slice(C), pk_ln_mlp_slab_floats(C));
        flush_line();
    }
    // one 32-row group per wave, four waves per workgroup; caps: forward / dx 512 workgroups = 65 536 rows, dw 256 (C = 32) = 32 768 rows,
    // 32 (C = 64) = 4 096 rows; a training-size M
    static const int kM[] = {1, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536, 65537, 196608};
    for (int which = 0; which < 3; ++which) {
        for (int C : {32, 64, 48}) for (int M : kM) mlp_call(which, M, C, 0, 0, kGood);
        for (int C : {32, 64}) for (int rps : {0, 49}) for (int sc = 0; sc < 2; ++sc) mlp_call(which, 129, C, rps, sc, kGood);
        each_pointer(13, [&](const Ptrs& P) { mlp_call(which, 4096, 64, 49, 1, P); });
        // M * C against the 32-bit refusal, and no rows
        for (int M : {33554431, 33554432}) mlp_call(which, M, 32, 0, 0, kGood);
        for (int M : {16777215, 16777216}) mlp_call(which, M, 64, 0, 0, kGood);
        for (int M : {0, -1}) mlp_call(which, M, 32, 0, 0, kGood);
        // two faults at once: which check comes first
        mlp_call(which, 0, 48, 0, 0, Ptrs{1, -1});          // unsupported C, no rows, x null
        mlp_call(which, 33554432, 32, 0, 1, kGood);         // scale without rows_per_sample, too large
        mlp_call(which, 33554432, 32, 0, 0, Ptrs{-1, 1});   // too large, x misaligned
        mlp_call(which, 4096, 32, 0, 0, Ptrs{4, 1});        // x misaligned, w1 null
        mlp_call(which, 4096, 32, 0, 1, Ptrs{2, -1});       // gamma null, scale without rows_per_sample
    }
}

// ---- fused MLP half, wide channels
static void mlpw_call(int M, int C, int c_real, int hidden, int rps, int sc, const Ptrs& P) {
    emit("mlp_wide M=%d C=%d c_real=%d hidden=%d rps=%d sc=%d null=%d mis=%d", M, C, c_real, hidden, rps, sc, P.null_at, P.mis_at);
    finish(pk_ln_mlp_wide_fwd(P(1), P.f<float>(2), P.f<float>(3), P(4), P.f<float>(5), P(6), P.f<float>(7), sc ? P.f<float>(9) : nullptr, P(8), M, C, c_real, hidden,
                              rps, 1e-5f, STREAM));
    emit(" supported=%d,%d", pk_ln_mlp_wide_supported(C, hidden, M), pk_ln_mlp_wide_supported(C, hidden, 0));
    flush_line();
}
static void sweep_mlp_wide() {
    // {C, the largest hidden that is staged once (slices * (fragments * 1024 + 128) <= 150 KiB), rows per workgroup}
    static const int kC[][3] = {{80, 416, 256}, {128, 288, 256}, {160, 224, 256}, {256, 128, 128}, {320, 96, 128}};
    for (auto& c : kC) {
        const int C = c[0], res = c[1], per_wg = c[2];
        for (int hidden : {32, res, res + 32, 4 * C, 2048, 2080, 40, 0, -32}) mlpw_call(4096, C, C, hidden, 0, 0, kGood);
        // rows: workgroup edges, the 160-workgroup rule of _wide_supported, the 256-CU cap of the staged-once grid, a training size
        for (int hidden : {res, res + 32})
            for (int M : {1, per_wg - 1, per_wg, per_wg + 1, 159 * per_wg, 159 * per_wg + 1, 160 * per_wg, 256 * per_wg - 1, 256 * per_wg, 256 * per_wg + 1, 196608})
                mlpw_call(M, C, C, hidden, 0, 0, kGood);
        for (int c_real : {0, 1, C - 1, C, C + 1, -1}) mlpw_call(4096, C, c_real, 4 * C, 0, 0, kGood);
    }
    for (int C : {32, 64, 96, 328, 0}) mlpw_call(4096, C, C, 4 * (C > 0 ? C : 32), 0, 0, kGood);
    for (int rps : {0, 49}) for (int sc = 0; sc < 2; ++sc) mlpw_call(4096, 80, 78, 320, rps, sc, kGood);
    each_pointer(10, [&](const Ptrs& P) { mlpw_call(4096, 160, 156, 640, 49, 1, P); });
    for (int M : {13421772, 13421773}) mlpw_call(M, 80, 80, 320, 0, 0, kGood);          // M * C against the 32-bit refusal
    for (int M : {0, -1}) mlpw_call(M, 80, 80, 320, 0, 0, kGood);
    mlpw_call(0, 96, 0, 384, 0, 1, Ptrs{1, -1});           // two faults at once: unsupported C first
    mlpw_call(4096, 80, 0, 320, 0, 0, Ptrs{1, -1});        // x null, c_real 0
    mlpw_call(4096, 80, 0, 320, 0, 1, kGood);              // c_real 0, scale without rows_per_sample
    mlpw_call(13421773, 80, 80, 320, 0, 1, kGood);         // scale without rows_per_sample, too large
    mlpw_call(13421773, 80, 80, 320, 0, 0, Ptrs{-1, 3});   // too large, beta misaligned
    for (int M : {0, 1, -1, 159 * 256, 159 * 256 + 1}) {
        emit("mlp_wide_supported M=%d:", M);
        for (int C : {80, 128, 160, 256, 320, 64}) for (int hidden : {32, 2048, 2080, 48}) emit(" %d", pk_ln_mlp_wide_supported(C, hidden, M));
        flush_line();
    }
}

// ---- fused attention half, C = 32 / 64
static void attn_call(int bwd, int nw, int wps, int heads, int C, int sc, int save, const Ptrs& P) {
    emit("%s nw=%d wps=%d heads=%d C=%d sc=%d save=%d null=%d mis=%d", bwd ? "attn_bwd" : "attn_fwd", nw, wps, heads, C, sc, save, P.null_at, P.mis_at);
    const float* scale = sc ? P.f<float>(10) : nullptr;
    if (bwd)
        finish(pk_attn_block_bwd(P(0), P(1), P.f<int32_t>(2), P.f<float>(3), P.f<float>(4), P.f<float>(5), P(6), P.f<float>(7), P(13), P(14), scale, P(11),
                                 P.f<float>(12), P(9), P(15), P(16), P.f<float>(17), P.f<float>(18), nw, wps, heads, C, 1e-5f, STREAM));
    else
        finish(pk_attn_block_fwd(P(1), P.f<int32_t>(2), P.f<float>(3), P.f<float>(4), P.f<float>(5), P(6), P.f<float>(7), P(8), P.f<float>(19), scale, P(9),
                                 (save & 1) ? P(11) : nullptr, (save & 2) ? P.f<float>(12) : nullptr, nw, wps, heads, C, 1e-5f, STREAM));
    emit(" blocks=%d supported=%d", pk_attn_block_blocks(nw), pk_attn_block_supported(C, heads));
    flush_line();
}
static void sweep_attn() {
    static const int kCH[][2] = {{32, 1}, {64, 2}, {64, 1}, {48, 1}, {32, 2}, {0, 0}};
    // one window per wave, four per workgroup, at most 256 workgroups; 1 000 000 windows are beyond the 32-bit refusal
    static const int kNW[] = {1, 3, 4, 5, 1023, 1024, 1025, 1000000};
    for (int bwd = 0; bwd < 2; ++bwd) {
        for (auto& ch : kCH) for (int nw : kNW) attn_call(bwd, nw, 0, ch[1], ch[0], 0, 3, kGood);
        for (int save = 0; save < 4; ++save) attn_call(bwd, 5, 0, 1, 32, 0, save, kGood);
        for (int C : {32, 64}) for (int wps : {0, 64}) for (int sc = 0; sc < 2; ++sc) attn_call(bwd, 1025, wps, C / 32, C, sc, 3, kGood);
        each_pointer(20, [&](const Ptrs& P) { attn_call(bwd, 1024, 64, 2, 64, 1, 3, P); });
        for (int nw : {228261, 228262}) attn_call(bwd, nw, 0, 1, 32, 0, 3, kGood);          // windows * 49 * 3C against the 32-bit refusal
        for (int nw : {114130, 114131}) attn_call(bwd, nw, 0, 2, 64, 0, 3, kGood);
        for (int nw : {0, -1}) attn_call(bwd, nw, 0, 1, 32, 0, 3, kGood);
        attn_call(bwd, 0, 0, 1, 48, 1, 3, Ptrs{1, -1});            // two faults at once: unsupported C first
        attn_call(bwd, 1024, 0, 1, 32, 1, 3, Ptrs{1, -1});         // x null, row_scale without windows_per_sample
        attn_call(bwd, 1024, 0, 1, 32, 1, 3, Ptrs{-1, 1});         // row_scale without windows_per_sample, x misaligned
        attn_call(bwd, 228262, 0, 1, 32, 0, 3, Ptrs{-1, 1});       // x misaligned, too large
    }
    emit("attn_blocks");
    for (int nw : {-1, 0, 1, 4, 5, 1020, 1021, 1024, 1025, 1 << 30}) emit(" %d", pk_attn_block_blocks(nw));
    flush_line();
}

// ---- fused attention half, head_dim 40
static void attnw_call(int nw, int wps, int heads, int C, int c_real, float ss, int sc, const Ptrs& P) {
    emit("attn_wide nw=%d wps=%d heads=%d C=%d c_real=%d ss=%a sc=%d null=%d mis=%d", nw, wps, heads, C, c_real, (double)ss, sc, P.null_at, P.mis_at);
    finish(pk_attn_block_wide_fwd(P(1), P.f<int32_t>(2), P.f<float>(3), P.f<float>(4), P.f<float>(5), P(6), P.f<float>(7), P(8), P.f<float>(19),
                                  sc ? P.f<float>(10) : nullptr, P(9), nw, wps, heads, C, c_real, ss, 1e-5f, STREAM));
    emit(" supported=%d,%d", pk_attn_block_wide_supported(C, heads, nw), pk_attn_block_wide_supported(C, heads, 0));
    flush_line();
}
static void sweep_attn_wide() {
    const float ss = 0.16012815f;          // 39^-0.5
    // one window per wave, eight per workgroup, at most 256 workgroups; _wide_supported wants 1 024 windows
    for (int nw : {1, 8, 9, 1023, 1024, 2047, 2048, 2049, 196608}) attnw_call(nw, 0, 2, 80, 78, ss, 0, kGood);
    static const int kCH[][2] = {{80, 1}, {80, 4}, {64, 2}, {160, 4}, {78, 2}, {0, 0}};
    for (auto& ch : kCH) attnw_call(2048, 0, ch[1], ch[0], ch[0], ss, 0, kGood);
    for (int c_real : {-1, 0, 1, 79, 80, 81}) attnw_call(2048, 0, 2, 80, c_real, ss, 0, kGood);
    for (float s : {-1.f, 0.f, 1e-30f, 1.f}) attnw_call(2048, 0, 2, 80, 78, s, 0, kGood);
    for (int wps : {0, 64}) for (int sc = 0; sc < 2; ++sc) attnw_call(2048, wps, 2, 80, 78, ss, sc, kGood);
    each_pointer(20, [&](const Ptrs& P) { attnw_call(2048, 64, 2, 80, 78, ss, 1, P); });
    for (int nw : {91304, 91305}) attnw_call(nw, 0, 2, 80, 78, ss, 0, kGood);          // windows * 49 * 3C against the 32-bit refusal
    for (int nw : {0, -1}) attnw_call(nw, 0, 2, 80, 78, ss, 0, kGood);
    attnw_call(0, 0, 1, 80, 0, ss, 1, Ptrs{1, -1});          // two faults at once: unsupported first
    attnw_call(2048, 0, 2, 80, 0, ss, 0, Ptrs{1, -1});       // x null, c_real 0
    attnw_call(2048, 0, 2, 80, 0, ss, 1, kGood);             // c_real 0, row_scale without windows_per_sample
    attnw_call(2048, 0, 2, 80, 78, ss, 1, Ptrs{-1, 1});      // row_scale without windows_per_sample, x misaligned
    attnw_call(91305, 0, 2, 80, 78, ss, 0, Ptrs{-1, 4});     // beta misaligned, too large
}

// ---- window-attention core
static void win_call(int bwd, int nw, int heads, int C, float ss, int opt, const Ptrs& P) {
    emit("%s nw=%d heads=%d C=%d ss=%a opt=%d null=%d mis=%d", bwd ? "win_bwd" : "win_fwd", nw, heads, C, (double)ss, opt, P.null_at, P.mis_at);
    if (bwd)
        finish(pk_window_attn_bwd(P(0), P.f<float>(1), P(2), P(3), P.f<float>(4), P(5), P.f<float>(6), opt ? P.f<float>(7) : nullptr, nw, heads, C, ss, STREAM));
    else
        finish(pk_window_attn_fwd(P(0), P.f<float>(1), P(2), opt ? P.f<float>(4) : nullptr, nw, heads, C, ss, STREAM));
    emit(" groups=%d ws_floats=%d", pk_window_attn_bwd_groups(nw, heads), pk_window_attn_bwd_ws_floats(nw, heads));
    flush_line();
}
static void sweep_window_attn() {
    for (int bwd = 0; bwd < 2; ++bwd) {
        // head dimensions on each side of the four dispatch arms (16 / 32 / 48), beyond 64, not a multiple of 8
        for (int heads : {1, 2}) for (int d : {8, 16, 24, 32, 40, 48, 56, 64, 72, 12, 4})
            for (int opt = 0; opt < 2; ++opt) win_call(bwd, 1000, heads, heads * d, 0.f, opt, kGood);
        for (float ss : {-1.f, 0.f, 0.25f}) win_call(bwd, 1000, 2, 64, ss, 1, kGood);
        static const int kBad[][2] = {{2, 33}, {3, 64}, {1, 12}, {3, 36}, {0, 32}, {2, 0}, {-1, 32}};          // {heads, C}
        for (auto& hc : kBad) win_call(bwd, 1000, hc[0], hc[1], 0.f, 1, kGood);
        // the group rule of the backward: 2 048 resident waves, ceil(windows * heads / 2 048) windows per workgroup
        for (int heads : {1, 2, 3}) for (int nw : {1, 682, 683, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 196608}) win_call(bwd, nw, heads, 32 * heads, 0.f, bwd, kGood);
        for (int nw : {0, -1}) win_call(bwd, nw, 2, 64, 0.f, 1, kGood);
        each_pointer(8, [&](const Ptrs& P) { win_call(bwd, 1000, 2, 64, 0.f, 1, P); });
    }
    emit("win_bwd_groups");
    static const int kNH[][2] = {{0, 2}, {2, 0}, {-1, 2}, {1000000, 8}, {2048, 1}, {2049, 1}, {1 << 30, 1}};
    for (auto& nh : kNH) emit(" %d", pk_window_attn_bwd_groups(nh[0], nh[1]));
    flush_line();
}

int main() {
    sweep_mlp();
    sweep_mlp_wide();
    sweep_attn();
    sweep_attn_wide();
    sweep_window_attn();
    return 0;
}
