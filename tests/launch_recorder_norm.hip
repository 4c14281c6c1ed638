// Host-only launch recorder for the normalisation, exchange-unit and layout units (tests/test_launch_routes_norm.py): every
// extern "C" entry of pk_bn.hip, pk_ln.hip, pk_exchange.hip and pk_layout.hip, swept over the smallest values at which each launch
// rule can go wrong.  One line per call: the problem, every launch with ALL its scalar and pointer arguments in order (so the
// launcher-computed rows_per_block, nb, inv_count, cchunks, split are there) and, for the grouped kernels, the per-member tables;
// the return code, the error text and the size queries for the same problem.
//
// Build: hipcc --offload-host-only -O1 -std=c++17 tests/launch_recorder_norm.hip -o launch_recorder_norm
// -DPK_NORM_SINGLE_UNIT='"/path/to/pk_norm.hip"' (with -I <csrc>) records from the single unit these four were split from.
#include "launch_recorder.h"

#include <type_traits>

#ifdef PK_NORM_SINGLE_UNIT
#include PK_NORM_SINGLE_UNIT
#else
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_bn.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_ln.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_exchange.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_layout.hip"
#endif

// ---- argument printers
static void rec_ptr(const void* p) { emit(" %lx", (unsigned long)(uintptr_t)p); }
static void rec_struct(const BnFwdGroup& g) {
    emit(" n=%d", g.n);
    for (int i = 0; i < g.n; ++i) {
        const PkBnFwdDesc& d = g.d[i];
        emit(" [%d ncg=%d rpb=%d rows=%lld tiles=%d C=%d relu=%d raw=%lx res=%lx mask=%lx]", g.first[i], g.ncg[i], g.rpb[i], (long long)d.rows, d.tiles, d.C,
             d.relu, (unsigned long)(uintptr_t)d.raw, (unsigned long)(uintptr_t)d.residual, (unsigned long)(uintptr_t)d.relu_mask);
    }
    emit(" end=%d", g.first[g.n]);
}
static void rec_struct(const BnBwdGroup& g) {
    emit(" n=%d", g.n);
    for (int i = 0; i < g.n; ++i) {
        const PkBnBwdDesc& d = g.d[i];
        emit(" [%d,%d nb=%d rpb_r=%d ncg=%d rpb_a=%d rows=%lld C=%d relu=%d dy=%lx y=%lx mask=%lx dres=%lx]", g.first_r[i], g.first_a[i], g.nb[i], g.rpb_r[i],
             g.ncg[i], g.rpb_a[i], (long long)d.rows, d.C, d.relu, (unsigned long)(uintptr_t)d.dy, (unsigned long)(uintptr_t)d.y_act,
             (unsigned long)(uintptr_t)d.relu_mask, (unsigned long)(uintptr_t)d.dresidual);
    }
    emit(" end=%d,%d", g.first_r[g.n], g.first_a[g.n]);
}
static void rec_struct(const FuseArgs& a) {
    emit(" {n=%d", a.n);
    for (int k = 0; k < 4; ++k) emit(" %lx:%dx%d", (unsigned long)(uintptr_t)a.in[k].p, a.in[k].H, a.in[k].W);
    emit(" out=%lx B=%d %dx%d C=%d relu=%d mask=%lx}", (unsigned long)(uintptr_t)a.out, a.B, a.H, a.W, a.C, a.relu, (unsigned long)(uintptr_t)a.mask_y);
}
static void rec_struct(const FuseGroup& g) {
    emit(" n=%d", g.n);
    for (int i = 0; i < g.n; ++i) {
        emit(" [%d", g.first[i]);
        rec_struct(g.a[i]);
        emit("]");
    }
    emit(" end=%d", g.first[g.n]);
}
static void rec_struct(const UpBwdGroup& g) {
    emit(" n=%d", g.n);
    for (int i = 0; i < g.n; ++i) {
        const PkUpBwdDesc& d = g.d[i];
        emit(" [%d split=%d B=%d %dx%d<-%dx%d C=%d dy=%lx mask=%lx dsrc=%lx]", g.first[i], g.split[i], d.B, d.Hs, d.Ws, d.H, d.W, d.C,
             (unsigned long)(uintptr_t)d.dy, (unsigned long)(uintptr_t)d.mask_y, (unsigned long)(uintptr_t)d.dsrc);
    }
    emit(" end=%d", g.first[g.n]);
}
template <class T> static void rec_val(const T& v) {
    if constexpr (std::is_pointer_v<T>) rec_ptr((const void*)v);
    else if constexpr (std::is_floating_point_v<T>) emit(" %.9g", (double)v);
    else if constexpr (std::is_integral_v<T>) emit(" %lld", (long long)v);
    else rec_struct(v);
}
template <class... A> static void rec_args(Rec, const A&... a) {
    emit(" a=");
    (rec_val(a), ...);
}
// k_sum_partials launched without its three defaulted trailing parameters: the kernel gets the defaults, print them
template <class P, class O>
static void rec_args(Rec, const P& part, const int& nb, const int& K, const int& stride, const O& out, const float& scale, const int& accumulate) {
    rec_args(Rec{}, part, nb, K, stride, out, scale, accumulate, (float*)nullptr, (float*)nullptr, 0);
}

// ---- made-up addresses, one region per argument position; `null_at` (0-based, -1: none) knocks one pointer out
struct Ptrs {
    int null_at;
    void* operator()(int k) const { return k == null_at ? nullptr : fake<void>(0x10000000u + 0x08000000u * (uintptr_t)k); }
    template <class T> T* as(int k) const { return (T*)(*this)(k); }
};
static const int64_t kRowsBn[] = {1, 31, 32, 33, 127, 128, 129, 2048, 2049, 4096, 4097, 16384, 16385, 32768, 32769, (1ll << 30) - 1, 1ll << 30};
static const int kCBn[] = {8, 32, 40, 256, 1024, 1032, 12};
// B, H, W with B*H*W = 1, 255, 256, 257, 2^19 - 1, 2^19, 2^19 + 1, 2^20 - 1, 2^20, 2^20 + 1, 2^32 - 2, 2^32 - 1
static const int kBHW[][3] = {{1, 1, 1}, {1, 15, 17}, {1, 16, 16}, {1, 1, 257}, {1, 1, 524287}, {1, 512, 1024}, {1, 3, 174763}, {1, 1025, 1023},
                              {1, 1024, 1024}, {1, 17, 61681}, {2, 1, 2147483647}, {1, 65535, 65537}};
static int64_t bhw(const int* t) { return (int64_t)t[0] * t[1] * t[2]; }

// ---- BatchNorm
static PkBnFwdDesc bnf_desc(int64_t rows, int tiles, int C, int opt, const Ptrs& P, uintptr_t off = 0) {
    PkBnFwdDesc d{};
    auto o = [&](int k) { void* p = P(k); return p ? (void*)((uintptr_t)p + off) : p; };
    d.raw = o(0); d.stats_partial = (const float*)o(1); d.gamma = (const float*)o(2); d.beta = (const float*)o(3);
    d.y = o(4); d.save_mean = (float*)o(5); d.save_rstd = (float*)o(6);
    d.running_mean = opt ? (float*)o(9) : nullptr; d.running_var = opt ? (float*)o(10) : nullptr; d.num_batches_tracked = opt ? (int64_t*)o(11) : nullptr;
    d.residual = opt ? o(12) : nullptr; d.relu_mask = opt ? (uint8_t*)o(13) : nullptr;
    d.rows = rows; d.tiles = tiles; d.C = C; d.momentum = 0.1f; d.eps = 1e-5f; d.relu = opt;
    return d;
}
static void bnf_call(int64_t rows, int tiles, int C, int opt, int null_at) {
    const Ptrs P{null_at};
    const PkBnFwdDesc d = bnf_desc(rows, tiles, C, opt, P);
    emit("bn_fwd rows=%lld tiles=%d C=%d opt=%d null=%d", (long long)rows, tiles, C, opt, null_at);
    finish(pk_bn_train_fwd(d.raw, d.stats_partial, tiles, C, rows, d.gamma, d.beta, d.running_mean, d.running_var, d.num_batches_tracked, d.momentum, d.eps,
                           d.residual, d.y, d.save_mean, d.save_rstd, P.as<float>(7), P.as<float>(8), d.relu, d.relu_mask, STREAM));
    flush_line();
    if (null_at >= 7) return;
    emit("bn_fwd_group1 rows=%lld tiles=%d C=%d opt=%d null=%d", (long long)rows, tiles, C, opt, null_at);
    finish(pk_bn_train_fwd_group(&d, 1, STREAM));
    flush_line();
}
static PkBnBwdDesc bnb_desc(int64_t rows, int C, int relu, int ym, int dres, const Ptrs& P, uintptr_t off = 0) {
    PkBnBwdDesc d{};
    auto o = [&](int k) { void* p = P(k); return p ? (void*)((uintptr_t)p + off) : p; };
    d.dy = o(0); d.raw = o(1); d.save_mean = (const float*)o(2); d.save_rstd = (const float*)o(3); d.gamma = (const float*)o(4);
    d.partial = (float*)o(5); d.dgamma = (float*)o(6); d.dbeta = (float*)o(7); d.dx = o(8);
    d.y_act = (ym & 1) ? o(10) : nullptr; d.relu_mask = (ym & 2) ? (const uint8_t*)o(11) : nullptr; d.dresidual = dres ? o(12) : nullptr;
    d.rows = rows; d.C = C; d.relu = relu;
    return d;
}
static void bnb_call(int64_t rows, int C, int relu, int ym, int dres, int null_at) {
    const Ptrs P{null_at};
    const PkBnBwdDesc d = bnb_desc(rows, C, relu, ym, dres, P);
    emit("bn_bwd rows=%lld C=%d relu=%d ym=%d dres=%d null=%d", (long long)rows, C, relu, ym, dres, null_at);
    finish(pk_bn_bwd(d.dy, d.y_act, d.raw, d.save_mean, d.save_rstd, d.gamma, d.partial, P.as<float>(9), d.dgamma, d.dbeta, d.dx, d.dresidual, rows, C, relu,
                     d.relu_mask, STREAM));
    emit(" blocks=%d group_blocks=%d", pk_bn_bwd_blocks(rows), pk_bn_bwd_group_blocks(rows));
    flush_line();
    if (null_at >= 9) return;
    emit("bn_bwd_group1 rows=%lld C=%d relu=%d ym=%d dres=%d null=%d", (long long)rows, C, relu, ym, dres, null_at);
    finish(pk_bn_bwd_group(&d, 1, STREAM));
    flush_line();
}
static const int kGroupN[] = {0, 1, 2, PK_GROUP_MAX, PK_GROUP_MAX + 1};
static void sweep_bn() {
    for (int64_t rows : kRowsBn) for (int C : kCBn) for (int tiles : {0, 1, 128, 129}) for (int opt = 0; opt < 2; ++opt) bnf_call(rows, tiles, C, opt, -1);
    for (int p = 0; p < 9; ++p) for (int tiles : {1, 129}) bnf_call(4096, tiles, 64, 0, p);
    for (int64_t rows : kRowsBn) for (int C : kCBn) for (int relu = 0; relu < 4; ++relu) for (int ym = 0; ym < 4; ++ym) for (int dres = 0; dres < 2; ++dres)
        bnb_call(rows, C, relu, ym, dres, -1);
    for (int C : {8, 16}) for (int64_t rows : {(1ll << 32) - 2, (1ll << 32) - 1, (1ll << 31) - 1, 1ll << 31}) bnb_call(rows / (C / 8), C, 1, 2, 0, -1);
    for (int p = 0; p < 10; ++p) for (int64_t rows : {4096, 65536}) bnb_call(rows, 64, 0, 0, 0, p);
    // groups: members of mixed sizes; `bad` 1 / 2 spoils the first / the last member (C not a multiple of 8)
    const Ptrs P{-1};
    for (int n : kGroupN) for (int bad = 0; bad < 3; ++bad) {
        if (bad && n < 2) continue;
        PkBnFwdDesc f[PK_GROUP_MAX + 1];
        PkBnBwdDesc b[PK_GROUP_MAX + 1];
        for (int i = 0; i <= PK_GROUP_MAX; ++i) {
            const int64_t rows = kRowsBn[(5 * i + 3) % 15];
            const int C = (bad == 1 && i == 0) || (bad == 2 && i == n - 1) ? 12 : kCBn[i % 5];
            f[i] = bnf_desc(rows, 1 + 40 * i, C, i & 1, P, (uintptr_t)i << 20);
            b[i] = bnb_desc(rows, C, i & 3, 1 + i % 3, i & 1, P, (uintptr_t)i << 20);
        }
        emit("bn_fwd_group n=%d bad=%d", n, bad);
        finish(pk_bn_train_fwd_group(f, n, STREAM));
        flush_line();
        emit("bn_bwd_group n=%d bad=%d", n, bad);
        finish(pk_bn_bwd_group(b, n, STREAM));
        flush_line();
    }
    emit("bn_group_null");
    finish(pk_bn_train_fwd_group(nullptr, 1, STREAM));
    finish(pk_bn_bwd_group(nullptr, 1, STREAM));
    flush_line();
    // pk_bn_finalize, pk_bn_act, pk_relu_bwd
    for (int C : {0, 1, 15, 16, 17}) for (int tiles : {0, 1, 300}) for (int count : {0, 5}) for (int run = 0; run < 2; ++run) {
        emit("bn_finalize C=%d tiles=%d count=%d run=%d", C, tiles, count, run);
        finish(pk_bn_finalize(P.as<float>(0), tiles, C, count, P.as<float>(1), P.as<float>(2), run ? P.as<float>(7) : nullptr, run ? P.as<float>(8) : nullptr,
                              run ? P.as<int64_t>(9) : nullptr, 0.1f, 1e-5f, P.as<float>(3), P.as<float>(4), P.as<float>(5), P.as<float>(6), STREAM));
        flush_line();
    }
    for (int p = 0; p < 7; ++p) {
        const Ptrs Q{p};
        emit("bn_finalize null=%d", p);
        finish(pk_bn_finalize(Q.as<float>(0), 4, 32, 100, Q.as<float>(1), Q.as<float>(2), nullptr, nullptr, nullptr, 0.1f, 1e-5f, Q.as<float>(3), Q.as<float>(4),
                              Q.as<float>(5), Q.as<float>(6), STREAM));
        flush_line();
    }
    for (auto& t : kBHW) for (int C : {8, 24, 12, 0}) for (int opt = 0; opt < 2; ++opt) {
        const int64_t rows = bhw(t) / (C == 24 ? 3 : 1) + (C == 24 && bhw(t) % 3 ? 1 : 0);
        emit("bn_act rows=%lld C=%d opt=%d", (long long)rows, C, opt);
        finish(pk_bn_act(P(0), P.as<float>(1), P.as<float>(2), opt ? P(4) : nullptr, P(3), rows, C, opt, opt ? P.as<uint8_t>(5) : nullptr, STREAM));
        flush_line();
    }
    for (int p = 0; p < 4; ++p) {
        const Ptrs Q{p};
        emit("bn_act null=%d", p);
        finish(pk_bn_act(Q(0), Q.as<float>(1), Q.as<float>(2), nullptr, Q(3), 100, 32, 0, nullptr, STREAM));
        flush_line();
    }
    emit("bn_act rows=0");
    finish(pk_bn_act(P(0), P.as<float>(1), P.as<float>(2), nullptr, P(3), 0, 32, 0, nullptr, STREAM));
    flush_line();
    for (auto& t : kBHW) for (int off : {0, 4}) {
        const int64_t numel = bhw(t) * 8 + off;
        emit("relu_bwd numel=%lld", (long long)numel);
        finish(pk_relu_bwd(P(0), P(1), P(2), numel, STREAM));
        flush_line();
    }
    for (int p = 0; p < 3; ++p) {
        const Ptrs Q{p};
        emit("relu_bwd null=%d", p);
        finish(pk_relu_bwd(Q(0), Q(1), Q(2), 4096, STREAM));
        flush_line();
    }
    emit("relu_bwd numel=0");
    finish(pk_relu_bwd(P(0), P(1), P(2), 0, STREAM));
    flush_line();
}

// ---- LayerNorm, column sums, partial sums
static void sweep_ln() {
    const Ptrs P{-1};
    static const int kC[] = {8, 16, 24, 32, 40, 64, 72, 128, 136, 256, 264, 512, 520, 1024, 1032, 0, 12};
    static const int64_t kRows[] = {1, 31, 32, 33, 32 * 1024, 32 * 1024 + 1};
    for (int C : kC) for (int cr = 0; cr < 4; ++cr) for (int64_t rows : kRows) {
        const int Cr = cr == 0 ? 0 : cr == 1 ? C : cr == 2 ? C - 2 : C + 1;
        emit("ln_fwd rows=%lld C=%d Cr=%d", (long long)rows, C, Cr);
        finish(pk_layernorm_fwd(P(0), P.as<float>(1), P.as<float>(2), P(3), P.as<float>(4), P.as<float>(5), rows, C, Cr, 1e-5f, STREAM));
        flush_line();
        for (int dgb = 0; dgb < 4; ++dgb) for (int dres = 0; dres < 2; ++dres) {
            emit("ln_bwd rows=%lld C=%d Cr=%d dgb=%d dres=%d", (long long)rows, C, Cr, dgb, dres);
            finish(pk_layernorm_bwd(P(0), P(1), P.as<float>(2), P.as<float>(3), P.as<float>(4), dres ? P(9) : nullptr, P(5), P.as<float>(6),
                                    (dgb & 1) ? P.as<float>(7) : nullptr, (dgb & 2) ? P.as<float>(8) : nullptr, rows, C, Cr, STREAM));
            emit(" blocks=%d", pk_ln_bwd_blocks(rows));
            flush_line();
        }
    }
    for (int p = 0; p < 7; ++p) {
        const Ptrs Q{p};
        emit("ln null=%d", p);
        if (p < 6) finish(pk_layernorm_fwd(Q(0), Q.as<float>(1), Q.as<float>(2), Q(3), Q.as<float>(4), Q.as<float>(5), 100, 64, 0, 1e-5f, STREAM));
        finish(pk_layernorm_bwd(Q(0), Q(1), Q.as<float>(2), Q.as<float>(3), Q.as<float>(4), nullptr, Q(5), Q.as<float>(6), nullptr, nullptr, 100, 64, 0, STREAM));
        flush_line();
    }
    emit("ln rows=0");
    finish(pk_layernorm_fwd(P(0), P.as<float>(1), P.as<float>(2), P(3), P.as<float>(4), P.as<float>(5), 0, 64, 0, 1e-5f, STREAM));
    finish(pk_layernorm_bwd(P(0), P(1), P.as<float>(2), P.as<float>(3), P.as<float>(4), nullptr, P(5), P.as<float>(6), nullptr, nullptr, 0, 64, 0, STREAM));
    emit(" blocks=%d,%d,%d", pk_ln_bwd_blocks(0), pk_ln_bwd_blocks(-5), pk_ln_bwd_blocks(1ll << 40));
    flush_line();
    for (int N : {8, 40, 2048, 2056, 12, 0}) for (int map = 0; map < 2; ++map) for (int sc = 0; sc < 2; ++sc) for (int rps : {0, 49}) for (int64_t rows : kRows) {
        emit("colsum rows=%lld N=%d map=%d sc=%d rps=%d", (long long)rows, N, map, sc, rps);
        finish(pk_colsum_bf16(P(0), map ? P.as<int32_t>(3) : nullptr, sc ? P.as<float>(4) : nullptr, rps, P.as<float>(1), P.as<float>(2), rows, N, STREAM));
        flush_line();
    }
    for (int p = 0; p < 3; ++p) {
        const Ptrs Q{p};
        emit("colsum null=%d", p);
        finish(pk_colsum_bf16(Q(0), nullptr, nullptr, 0, Q.as<float>(1), Q.as<float>(2), 100, 64, STREAM));
        flush_line();
    }
    emit("colsum rows=0");
    finish(pk_colsum_bf16(P(0), nullptr, nullptr, 0, P.as<float>(1), P.as<float>(2), 0, 64, STREAM));
    flush_line();
    for (int K : {0, 1, 15, 16, 17}) for (int nb : {0, 1, 64, 1024}) for (int ds : {-1, 0, 3}) for (int acc = 0; acc < 2; ++acc) {
        emit("sum_partials K=%d nb=%d stride=%d acc=%d", K, nb, K + ds, acc);
        finish(pk_sum_partials(P.as<float>(0), nb, K, K + ds, P.as<float>(1), 0.5f, acc, STREAM));
        flush_line();
    }
    for (int p = 0; p < 2; ++p) {
        const Ptrs Q{p};
        emit("sum_partials null=%d", p);
        finish(pk_sum_partials(Q.as<float>(0), 4, 16, 16, Q.as<float>(1), 1.f, 0, STREAM));
        flush_line();
    }
}

// ---- exchange unit
static PkFuseDesc fuse_desc(const int* t, int C, int n_in, int shape, int mask, int relu, const Ptrs& P, uintptr_t off = 0) {
    PkFuseDesc d{};
    // shape 0: input i at 1 / 2^i of the output; 1: all at the output's size; 2: the LAST input one row taller than the output;
    // 3: the FIRST input at half the output's size
    for (int i = 0; i < 4; ++i) {
        int sh = shape == 1 ? 0 : i;
        if (shape == 3 && i == 0) sh = 1;
        d.inputs[i] = i < n_in || n_in > 4 ? (const void*)((uintptr_t)P(i) + off) : nullptr;
        d.in_h[i] = (t[1] >> sh) > 0 ? t[1] >> sh : 1;
        d.in_w[i] = (t[2] >> sh) > 0 ? t[2] >> sh : 1;
        if (shape == 2 && i == n_in - 1) d.in_h[i] = t[1] + 1;
        if (!P(i)) d.inputs[i] = nullptr;
    }
    d.n_inputs = n_in; d.out = P(4) ? (void*)((uintptr_t)P(4) + off) : nullptr; d.mask_y = mask ? (const void*)((uintptr_t)P(5) + off) : nullptr;
    d.B = t[0]; d.H = t[1]; d.W = t[2]; d.C = C; d.relu = relu;
    return d;
}
static void fuse_call(const int* t, int C, int n_in, int shape, int mask, int relu, int null_at) {
    const Ptrs P{null_at};
    const PkFuseDesc d = fuse_desc(t, C, n_in, shape, mask, relu, P);
    if (!mask) {
        emit("fuse B=%d %dx%d C=%d n=%d shape=%d relu=%d null=%d", t[0], t[1], t[2], C, n_in, shape, relu, null_at);
        finish(pk_fuse_sum(null_at == 6 ? nullptr : d.inputs, null_at == 7 ? nullptr : d.in_h, null_at == 8 ? nullptr : d.in_w, n_in, d.out, d.B, d.H, d.W, C, relu,
                           STREAM));
        flush_line();
        if (null_at >= 6) return;
    }
    emit("fuse_group1 B=%d %dx%d C=%d n=%d shape=%d mask=%d relu=%d null=%d", t[0], t[1], t[2], C, n_in, shape, mask, relu, null_at);
    finish(pk_fuse_sum_group(&d, 1, STREAM));
    flush_line();
}
static PkUpBwdDesc up_desc(int B, int H, int W, int Hs, int Ws, int C, int mask, const Ptrs& P, uintptr_t off = 0) {
    PkUpBwdDesc d{};
    d.dy = P(0) ? (const void*)((uintptr_t)P(0) + off) : nullptr; d.dsrc = P(1) ? (void*)((uintptr_t)P(1) + off) : nullptr;
    d.mask_y = mask ? (const void*)((uintptr_t)P(2) + off) : nullptr;
    d.B = B; d.H = H; d.W = W; d.Hs = Hs; d.Ws = Ws; d.C = C;
    return d;
}
static void up_call(int B, int64_t H, int64_t W, int Hs, int Ws, int C, int null_at) {
    if (H > 0x7fffffff || W > 0x7fffffff) return;
    const Ptrs P{null_at};
    const PkUpBwdDesc d = up_desc(B, (int)H, (int)W, Hs, Ws, C, 0, P);
    emit("up_bwd B=%d %dx%d<-%lldx%lld C=%d null=%d", B, Hs, Ws, (long long)H, (long long)W, C, null_at);
    finish(pk_upsample_bilinear_bwd(d.dy, d.dsrc, B, d.H, d.W, Hs, Ws, C, STREAM));
    flush_line();
    for (int mask = 0; mask < 2; ++mask) {
        const PkUpBwdDesc m = up_desc(B, (int)H, (int)W, Hs, Ws, C, mask, P);
        emit("up_bwd_group1 B=%d %dx%d<-%lldx%lld C=%d mask=%d null=%d", B, Hs, Ws, (long long)H, (long long)W, C, mask, null_at);
        finish(pk_upsample_bwd_group(&m, 1, STREAM));
        flush_line();
    }
}
static void sweep_exchange() {
    for (auto& t : kBHW) for (int C : {8, 16, 12, 0}) {
        if (C == 16 && bhw(t) > (1ll << 31)) continue;
        fuse_call(t, C, 1, 1, 0, 0, -1);
        fuse_call(t, C, 1, 1, 1, 1, -1);
    }
    static const int small[3] = {2, 16, 12}, odd[3] = {1, 7, 5};
    for (const int* t : {small, odd}) for (int n_in : {0, 1, 2, 4, 5}) for (int shape = 0; shape < 4; ++shape) for (int mask = 0; mask < 2; ++mask) for (int relu = 0; relu < 2; ++relu)
        fuse_call(t, 32, n_in, shape, mask, relu, -1);
    for (int p = 0; p < 9; ++p) fuse_call(small, 32, 4, 0, 0, 0, p);
    static const int zeros[][3] = {{0, 16, 12}, {2, 0, 12}, {2, 16, 0}};
    for (auto& t : zeros) fuse_call(t, 32, 1, 1, 0, 0, -1);
    for (int r : {1, 2, 3, 4, 7, 8, 16}) for (int C : {8, 32}) {
        up_call(2, 6 * r, 5 * r, 6, 5, C, -1);
        up_call(2, 6 * r - (r > 1), 5 * r, 6, 5, C, -1);          // a ratio that is not whole: ry = ceil(H / Hs)
    }
    for (auto& t : kBHW) for (int r : {1, 4, 8}) up_call(t[0], (int64_t)t[1] * r, (int64_t)t[2] * r, t[1], t[2], 8, -1);
    for (int r : {4, 8, 16}) for (int Ws : {511, 512, 513}) up_call(1, 512 * r, Ws * r, 512, Ws, 8, -1);          // chunks * split at the block caps
    for (int r : {4, 8, 16}) for (int Ws : {255, 256, 257, 127, 128, 129, 63, 64, 65}) up_call(1, 512 * r, Ws * r, 512, Ws, 8, -1);
    up_call(2, 5, 10, 6, 5, 8, -1);          // H < Hs
    up_call(2, 12, 4, 6, 5, 8, -1);          // W < Ws
    up_call(0, 12, 10, 6, 5, 8, -1);
    up_call(2, 12, 10, 0, 5, 8, -1);
    up_call(2, 12, 10, 6, 0, 8, -1);
    up_call(2, 12, 10, 6, 5, 12, -1);
    up_call(2, 12, 10, 6, 5, 0, -1);
    for (int p = 0; p < 2; ++p) up_call(2, 12, 10, 6, 5, 8, p);
    // groups of mixed members; `bad` 1 / 2 spoils the first / the last member
    const Ptrs P{-1};
    for (int n : kGroupN) for (int bad = 0; bad < 3; ++bad) {
        if (bad && n < 2) continue;
        PkFuseDesc f[PK_GROUP_MAX + 1];
        PkUpBwdDesc u[PK_GROUP_MAX + 1];
        for (int i = 0; i <= PK_GROUP_MAX; ++i) {
            const bool spoil = (bad == 1 && i == 0) || (bad == 2 && i == n - 1);
            const int t[3] = {2 + (i & 1) * 62, 64 >> (i % 4), 48 >> (i % 4)};
            f[i] = fuse_desc(t, 32 << (i % 4), 1 + i % 4, spoil ? 2 : 0, !spoil && i % 3 == 0, i & 1, P, (uintptr_t)i << 20);
            const int r = 1 << (i % 5);
            u[i] = up_desc(t[0], t[1] * r, spoil ? t[2] - 1 : t[2] * r, t[1], t[2], 32 << (i % 4), i & 1, P, (uintptr_t)i << 20);
        }
        f[PK_GROUP_MAX - 2].B = 2; f[PK_GROUP_MAX - 2].H = 1024; f[PK_GROUP_MAX - 2].W = 1024;          // one member beyond the grouped block cap
        u[PK_GROUP_MAX - 2] = up_desc(2, 1024, 1024, 1024, 1024, 32, 0, P);
        emit("fuse_group n=%d bad=%d", n, bad);
        finish(pk_fuse_sum_group(f, n, STREAM));
        flush_line();
        emit("up_bwd_group n=%d bad=%d", n, bad);
        finish(pk_upsample_bwd_group(u, n, STREAM));
        flush_line();
    }
    emit("exchange_group_null");
    finish(pk_fuse_sum_group(nullptr, 1, STREAM));
    finish(pk_upsample_bwd_group(nullptr, 1, STREAM));
    flush_line();
    emit("sizeof_group_desc");
    for (int w = -1; w <= 6; ++w) emit(" %d", pk_sizeof_group_desc(w));
    flush_line();
}

// ---- layout conversion, weight packing, padded-twin copy (their descriptor tables are device memory the host never reads)
static void sweep_layout() {
    const Ptrs P{-1};
    for (auto& t : kBHW) for (int sp = 0; sp < 2; ++sp) {
        emit("nchw B=%d %dx%d sp=%d", t[0], t[1], t[2], sp);
        finish(pk_nchw_f32_to_nhwc_bf16(P.as<float>(0), sp ? P.as<float>(2) : nullptr, P(1), t[0], 3, t[1], t[2], 8, STREAM));
        flush_line();
    }
    static const int bad[][5] = {{0, 3, 4, 4, 8}, {1, 0, 4, 4, 8}, {1, 3, 0, 4, 8}, {1, 3, 4, 0, 8}, {1, 9, 4, 4, 8}, {1, 3, 4, 4, 12}, {1, 16, 4, 4, 16}, {1, 3, 4, 4, 0}};
    for (auto& b : bad) {
        emit("nchw B=%d Cin=%d %dx%d Cpad=%d", b[0], b[1], b[2], b[3], b[4]);
        finish(pk_nchw_f32_to_nhwc_bf16(P.as<float>(0), nullptr, P(1), b[0], b[1], b[2], b[3], b[4], STREAM));
        flush_line();
    }
    for (int p = 0; p < 2; ++p) {
        const Ptrs Q{p};
        emit("nchw null=%d", p);
        finish(pk_nchw_f32_to_nhwc_bf16(Q.as<float>(0), nullptr, Q(1), 1, 3, 4, 4, 8, STREAM));
        flush_line();
    }
    for (int nb : {-1, 0, 1, 1000, 1 << 24}) {
        emit("pack_weights n_blocks=%d", nb);
        finish(pk_pack_weights(P(0), P(1), P.as<int32_t>(2), P.as<int32_t>(3), nb, STREAM));
        flush_line();
        for (int dir = -1; dir <= 3; ++dir) {
            emit("embed_boxes n_blocks=%d dir=%d", nb, dir);
            finish(pk_embed_boxes(P.as<float>(0), P(1), P.as<int>(2), P.as<int>(3), nb, dir, STREAM));
            flush_line();
        }
    }
    for (int p = 0; p < 4; ++p) {
        const Ptrs Q{p};
        emit("pack_embed null=%d", p);
        finish(pk_pack_weights(Q(0), Q(1), Q.as<int32_t>(2), Q.as<int32_t>(3), 5, STREAM));
        finish(pk_embed_boxes(Q.as<float>(0), Q(1), Q.as<int>(2), Q.as<int>(3), 5, 1, STREAM));
        flush_line();
    }
}

int main() {
    sweep_bn();
    sweep_ln();
    sweep_exchange();
    sweep_layout();
    return 0;
}
