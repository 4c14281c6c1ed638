// Host-only launch recorder for the implicit-GEMM and weight-gradient units (tests/test_launch_routes.py).
//
// The two units are compiled into this program with the HIP launch macro replaced by a printer, so the real entry points run their
// argument checks and their routing on any machine and no kernel is ever started: hipGetDevice fails (the CU count takes its 256
// fallback), every pointer is a made-up address of a chosen alignment and nothing is dereferenced.  One output line per call:
// the problem, every launch (kernel, grid, block, LDS bytes, the fields of the argument block that the launcher fills in), the
// return code, the error text, and the values of the size queries for the same problem.  The test compares the output with
// tests/golden/launch_routes.txt.xz line for line: which kernel, tile and grid a shape gets is part of the library's behaviour.
//
// Build: hipcc --offload-host-only -O1 -std=c++17 tests/launch_recorder.hip -o launch_recorder
#include "launch_recorder.h"

// launcher-set fields, one overload per argument-block type
static void rec_args(Rec, const float* part, float* const&, int S, int, int, int, int layout, const float* bias_part, float* const&, int n_bias, int w_blocks) {
    emit(" S=%d layout=%d bias_off=%ld n_bias=%d w_blocks=%d", S, layout, bias_part ? (long)(bias_part - part) : -1L, n_bias, w_blocks);
}

#include "../infantposeestimation_gaussianbias_amd/csrc/pk_igemm.hip"
#include "../infantposeestimation_gaussianbias_amd/csrc/pk_wgrad.hip"

static void rec_args(Rec, const IgemmArgs& a) { emit(" v8=%d xr=%d cm=%d dg=%d", a.vec8, a.xcd_remap, a.chunk_major, a.dil_group); }
static void rec_args(Rec, const IgemmArgs& a, const int& pieces_per_wave) {
    rec_args(Rec{}, a);
    emit(" pp=%d", pieces_per_wave);
}
static void rec_args(Rec, const IgemmGroup& g) {
    emit(" n=%d", g.n);
    for (int i = 0; i < g.n; ++i) {
        emit(" [%d gy=%d", g.first[i], g.gy[i]);
        rec_args(Rec{}, g.a[i]);
        emit("]");
    }
    emit(" end=%d", g.first[g.n]);
}
static void rec_args(Rec, const WgradArgs& a) {
    emit(" ct=%d nt3=%d ns3=%d mps=%d bias_off=%ld", a.ctiles, a.ntiles3, a.nslices3, a.m_per_slice, a.bias_part ? (long)(a.bias_part - a.part) : -1L);
}
static void rec_args(Rec, const WgradGroup& g) {
    emit(" n=%d", g.n);
    for (int i = 0; i < g.n; ++i) {
        emit(" [%d", g.first[i]);
        rec_args(Rec{}, g.a[i]);
        emit("]");
    }
    emit(" end=%d", g.first[g.n]);
}

// made-up addresses: 16-byte aligned unless an offset is added
enum : uintptr_t { X_ = 0x10000000, W_ = 0x18000000, OUT_ = 0x20000000, STATS_ = 0x28000000, BIAS_ = 0x30000000, SCALE_ = 0x31000000,
                   RES_ = 0x38000000, MAP_ = 0x40000000, PRE_ = 0x48000000, WS_ = 0x50000000, DW_ = 0x58000000, DB_ = 0x5c000000 };

static void set_switches(int sw) {        // 0: defaults, 1: both thresholds at one tile, 2: both specialised kernels off
    unsetenv("PK_CONV8P"); unsetenv("PK_CONV8P_MIN_TILES"); unsetenv("PK_CONV3H"); unsetenv("PK_CONV3H_MIN_TILES");
    if (sw == 1) { setenv("PK_CONV8P_MIN_TILES", "1", 1); setenv("PK_CONV3H_MIN_TILES", "1", 1); }
    if (sw == 2) { setenv("PK_CONV8P", "0", 1); setenv("PK_CONV3H", "0", 1); }
}

// The full cross product of the conv axes has 16 million members.  Every value of every axis is kept and the product is thinned:
// the `core` sub-product (the axes that pick the kernel, everything else at its default) in full, the rest one member in `keep_1_in`,
// chosen by a fixed hash of the member's index.
static bool sampled(uint32_t index, uint32_t keep_1_in) {
    uint32_t h = index * 2654435761u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    return h % keep_1_in == 0;
}

static const int kB[] = {1, 2, 32, 64};
static const int kHW[][2] = {{64, 48}, {32, 24}, {16, 12}, {8, 6}, {96, 72}, {7, 5}};
static const int kC[] = {8, 32, 48, 64, 128, 256, 512};
static const int kLinM[] = {49, 3136, 25088, 200704};
static const int kLinC[] = {32, 64, 96, 128, 256, 512};

struct Geo { int B, Hs, Ws, Cin, Cout, k, s, dil, Ho, Wo; };
static Geo geo(int B, int H, int W, int ci, int co, int k, int s, int dil) {
    Geo g{B, H, W, ci, co, k, s, dil, 0, 0};
    if (dil) { g.Ho = 2 * H - (H & 1); g.Wo = 2 * W - (W & 1); }        // stride-2 data gradient: even and odd forward input sizes
    else { g.Ho = (H + 2 * (k / 2) - k) / s + 1; g.Wo = (W + 2 * (k / 2) - k) / s + 1; }
    return g;
}
template <class F> static void for_each_geo(bool with_dilated, F f) {
    for (int B : kB) for (auto& hw : kHW) for (int ci : kC) for (int co : kC) for (int k = 1; k <= 3; k += 2) for (int s = 1; s <= 2; ++s)
        for (int dil = 0; dil <= (with_dilated ? 1 : 0); ++dil) f(geo(B, hw[0], hw[1], ci, co, k, s, dil));
}

// The calls behind the problem lines (the line's head is emitted by the caller).  Option values beyond the sweeps' are for the case mode:
// ad / re 2: addend / residual 8 bytes off a 16-byte boundary; maps 2: a_rowmap only, 3: o_rowmap only; pg 3: preact_out 8 bytes off;
// re (linear): residual with a per-sample scale.
static void conv_call(const Geo& g, int st, int ad, int bi, int act, int om, int oa) {
    finish(pk_conv2d_nhwc(fake<void>(X_), fake<void>(W_), fake<void>(OUT_, oa ? 8 : 0), st ? fake<float>(STATS_) : nullptr,
                          bi ? fake<float>(BIAS_, bi == 2 ? 4 : 0) : nullptr, g.B, g.Hs, g.Ws, g.Cin, g.Cout, g.k, g.s, g.dil, g.Ho, g.Wo,
                          act, om, ad ? fake<void>(RES_, ad == 2 ? 8 : 0) : nullptr, STREAM));
    emit(" rows=%d", pk_conv_stats_rows(g.B, g.Hs, g.Ws, g.Cin, g.Cout, g.k, g.s, g.Ho, g.Wo));
    flush_line();
}
static void affine_call(const Geo& g, int re, int sc, int relu, int oa) {
    finish(pk_conv2d_affine_nhwc(fake<void>(X_), fake<void>(W_), fake<void>(OUT_, oa ? 8 : 0), sc ? fake<float>(SCALE_, sc == 2 ? 4 : 0) : nullptr,
                                 sc ? fake<float>(BIAS_, sc == 2 ? 4 : 0) : nullptr, re ? fake<void>(RES_, re == 2 ? 8 : 0) : nullptr, relu, g.B, g.Hs, g.Ws,
                                 g.Cin, g.Cout, g.k, g.s, g.Ho, g.Wo, STREAM));
    flush_line();
}
static void linear_call(int M, int N, int K, int maps, int pg, int act, int f32, int re, int rps) {
    finish(pk_linear_bf16(fake<void>(X_), fake<void>(W_), fake<void>(OUT_), fake<float>(BIAS_), re ? fake<void>(RES_, re == 2 ? 8 : 0) : nullptr,
                          re ? fake<float>(SCALE_) : nullptr, maps == 1 || maps == 2 ? fake<int32_t>(MAP_) : nullptr,
                          maps == 1 || maps == 3 ? fake<int32_t>(MAP_, 0x1000000) : nullptr, pg == 1 || pg == 3 ? fake<void>(PRE_, pg == 3 ? 8 : 0) : nullptr,
                          pg == 2 ? fake<void>(PRE_) : nullptr, M, N, K, rps, act, f32, STREAM));
    flush_line();
}

static void sweep_conv() {
    uint32_t index = 0;
    for_each_geo(true, [&](const Geo& g) {
        for (int sw = 0; sw < 3; ++sw) for (int st = 0; st < 2; ++st) for (int ad = 0; ad < 2; ++ad) for (int bi = 0; bi < 3; ++bi)
            for (int act = 0; act < 4; ++act) for (int om = 0; om < 3; ++om) for (int oa = 0; oa < 2; ++oa) {
                const bool core = !ad && !bi && !act && !om && !oa;
                if (!core && !sampled(index++, 192)) continue;
                set_switches(sw);
                emit("conv B=%d %dx%d ci=%d co=%d k=%d s=%d d=%d sw=%d st=%d ad=%d bi=%d act=%d om=%d oa=%d", g.B, g.Hs, g.Ws, g.Cin, g.Cout, g.k, g.s,
                     g.dil, sw, st, ad, bi, act, om, oa);
                conv_call(g, st, ad, bi, act, om, oa);
            }
    });
    index = 0;
    for_each_geo(false, [&](const Geo& g) {
        for (int sw = 0; sw < 3; ++sw) for (int re = 0; re < 2; ++re) for (int sc = 0; sc < 3; ++sc) for (int relu = 0; relu < 2; ++relu)
            for (int oa = 0; oa < 2; ++oa) {
                const bool core = sc == 1 && !relu && !oa;
                if (!core && !sampled(index++, 24)) continue;
                set_switches(sw);
                emit("affine B=%d %dx%d ci=%d co=%d k=%d s=%d sw=%d re=%d sc=%d relu=%d oa=%d", g.B, g.Hs, g.Ws, g.Cin, g.Cout, g.k, g.s, sw, re, sc, relu, oa);
                affine_call(g, re, sc, relu, oa);
            }
    });
    set_switches(0);
}

static void sweep_linear() {
    for (int M : kLinM) for (int N : kLinC) for (int K : kLinC) for (int maps = 0; maps < 2; ++maps) for (int pg = 0; pg < 3; ++pg)
        for (int act = 0; act < 2; ++act) for (int f32 = 0; f32 < 2; ++f32) {
            emit("linear M=%d N=%d K=%d maps=%d pg=%d act=%d f32=%d", M, N, K, maps, pg, act, f32);      // pg: 1 = preact out, 2 = gelu_of in
            linear_call(M, N, K, maps, pg, act, f32, 0, 0);
        }
}

static void wgrad_call(const char* tag, int M, int N, int Cin, int k, int s, int B, int Hs, int Ws, int Ho, int Wo, int flags, int nb, int dw) {
    emit("%s M=%d N=%d ci=%d k=%d s=%d B=%d %dx%d->%dx%d fl=%d nb=%d dw=%d", tag, M, N, Cin, k, s, B, Hs, Ws, Ho, Wo, flags, nb, dw);
    finish(pk_wgrad_bf16(fake<void>(X_), fake<void>(OUT_), fake<float>(WS_), dw ? fake<float>(DW_) : nullptr, (dw && nb) ? fake<float>(DB_) : nullptr, nb,
                         (flags & 1) ? fake<int32_t>(MAP_) : nullptr, (flags & 2) ? fake<int32_t>(MAP_, 0x1000000) : nullptr,
                         (flags & 4) ? fake<float>(SCALE_) : nullptr, (flags & 4) ? (Hs > 0 ? Hs * Ws : 49) : 0, M, N, Cin, k, s, B, Hs, Ws, Ho, Wo, dw ? 1 : 0,
                         STREAM));
    emit(" S=%d", pk_wgrad_slices(M, N, Cin, k, s, Hs, Ws, flags));
    flush_line();
}
static void sweep_wgrad() {
    uint32_t index = 0;
    for_each_geo(false, [&](const Geo& g) {
        for (int fl = 0; fl < 8; ++fl) for (int nb = 0; nb < 2; ++nb) for (int dw = 0; dw < 2; ++dw) {
            const bool core = !fl && !nb && !dw;
            if (!core && !sampled(index++, 12)) continue;
            wgrad_call("wgrad", g.B * g.Ho * g.Wo, g.Cout, g.Cin, g.k, g.s, g.B, g.Hs, g.Ws, g.Ho, g.Wo, fl, nb ? g.Cout : 0, dw);
        }
    });
    for (int M : kLinM) for (int N : kLinC) for (int K : kLinC) for (int fl = 0; fl < 8; ++fl) for (int grid = 0; grid < 2; ++grid)
        for (int nb = 0; nb < 2; ++nb) for (int dw = 0; dw < 2; ++dw) {
            const int B = M == 49 ? 1 : M / 3136, HW = M == 49 ? 7 : 56;          // M = B * ceil(H / 7) * ceil(W / 7) * 49
            wgrad_call("wlin", M, N, K, 1, 1, grid ? B : 0, grid ? HW : 0, grid ? HW : 0, 0, 0, fl, nb ? N : 0, dw);
        }
}

// groups: members of mixed channel counts and map sizes, all of one kind; `spoil` makes the last member of another kind
static void sweep_groups() {
    static const int chs[2][6] = {{32, 64, 128, 256, 48, 8}, {64, 128, 256, 128, 64, 256}};          // the second row allows the deep K-step
    const int sizes[] = {1, 3, PK_GROUP_MAX};
    for (int n : sizes) for (int B = 2; B <= 64; B *= 32) for (int k = 1; k <= 3; k += 2) for (int s = 1; s <= 2; ++s) for (int dil = 0; dil < 2; ++dil)
        for (int deep = 0; deep < 2; ++deep) for (int flavour = 0; flavour < 3; ++flavour) for (int spoil = 0; spoil < 2; ++spoil) {
            if (spoil && (n != 3 || flavour != 2)) continue;          // flavour 0: statistics, 1: scale / shift / residual / ReLU, 2: plain
            const int* ch = chs[deep];
            PkConvDesc d[PK_GROUP_MAX] = {};
            for (int i = 0; i < n; ++i) {
                const int* hw = kHW[i % 4];
                const Geo g = geo(B, hw[0], hw[1], ch[i % 6], ch[(i + 2 + i / 6) % 6], k, s, spoil && i == n - 1 ? !dil : dil);
                d[i].x = fake<void>(X_, i << 20); d[i].w = fake<void>(W_, i << 20); d[i].out = fake<void>(OUT_, i << 20);
                d[i].stats = flavour == 0 ? fake<float>(STATS_, i << 20) : nullptr;
                d[i].col_scale = flavour == 1 ? fake<float>(SCALE_, i << 12) : nullptr;
                d[i].bias = flavour == 1 ? fake<float>(BIAS_, i << 12) : nullptr;
                d[i].res = flavour == 1 || (dil && (i & 1)) ? fake<void>(RES_, (i << 20) + ((i & 2) ? 8 : 0)) : nullptr;
                d[i].B = g.B; d[i].Hs = g.Hs; d[i].Ws = g.Ws; d[i].Cin = g.Cin; d[i].Cout = g.Cout; d[i].ksize = k; d[i].stride = s;
                d[i].dilated_input = g.dil; d[i].Ho = g.Ho; d[i].Wo = g.Wo; d[i].act = flavour == 1 ? 3 : 0;
            }
            emit("cgroup n=%d B=%d k=%d s=%d d=%d deep=%d fv=%d spoil=%d", n, B, k, s, dil, deep, flavour, spoil);
            finish(pk_conv2d_group(d, n, STREAM));
            flush_line();
        }
    for (int n : sizes) for (int B = 2; B <= 64; B *= 32) for (int kind = 0; kind < 3; ++kind) for (int spoil = 0; spoil < 2; ++spoil) {
        if (spoil && n != 3) continue;
        PkWgradDesc d[PK_GROUP_MAX] = {};
        const int* ch = chs[0];
        emit("wgroup n=%d B=%d kind=%d spoil=%d S=", n, B, kind, spoil);          // kind 0: 1x1 stride 1, 1: 3x3 stride 2, 2: 3x3 stride 1 (not a group kind)
        for (int i = 0; i < n; ++i) {
            const int* hw = kHW[i % 4];
            const int kd = spoil && i == n - 1 ? !kind : kind;
            const Geo g = geo(B, hw[0], hw[1], ch[i % 6], ch[(i + 2 + i / 6) % 6], kd == 0 ? 1 : 3, kd == 1 ? 2 : 1, 0);
            d[i].x = fake<void>(X_, i << 20); d[i].grad_out = fake<void>(OUT_, i << 20); d[i].workspace = fake<float>(WS_, i << 22);
            d[i].B = g.B; d[i].Hs = g.Hs; d[i].Ws = g.Ws; d[i].Ho = g.Ho; d[i].Wo = g.Wo; d[i].N = g.Cout; d[i].Cin = g.Cin; d[i].ksize = g.k; d[i].stride = g.s;
            emit("%s%d", i ? "," : "", pk_wgrad_group_slices(g.B * g.Ho * g.Wo, g.Cout, g.Cin, g.k, g.s));
        }
        finish(pk_wgrad_group(d, n, STREAM));
        flush_line();
    }
    emit("group_limit");
    PkConvDesc c[1] = {};
    finish(pk_conv2d_group(c, PK_GROUP_MAX + 1, STREAM));
    PkWgradDesc w[1] = {};
    finish(pk_wgrad_group(w, PK_GROUP_MAX + 1, STREAM));
    flush_line();
}

// ---- case mode: problems from stdin, one per line, in the key=value form of the lines above; one record per input line.
//   switches sw=S
//   conv B= HxW ci= co= k= s= d= st= ad= bi= act= om= oa= [Ho= Wo=]          (Ho / Wo: a dilated output size other than the sweep's)
//   affine B= HxW ci= co= k= s= re= sc= relu= oa=
//   linear M= N= K= maps= pg= act= f32= [re= rps=]
//   cgroup n= m=B,Hs,Ws,Cin,Cout,k,s,d,Ho,Wo,stats,scale,res,act ...          (res 2: 8 bytes off a 16-byte boundary)
static int field(const char* line, const char* key, int dflt) {
    const size_t n = strlen(key);
    for (const char* c = line; (c = strstr(c, key)); c += n)
        if ((c == line || c[-1] == ' ') && c[n] == '=') return atoi(c + n + 1);
    return dflt;
}
static Geo line_geo(const char* line, int dil) {
    int H = 0, W = 0;
    for (const char* c = line; (c = strchr(c, ' ')); ) {
        ++c;
        if (sscanf(c, "%dx%d", &H, &W) == 2 && H > 0 && W > 0) break;
    }
    Geo g = geo(field(line, "B", 1), H, W, field(line, "ci", 8), field(line, "co", 8), field(line, "k", 1), field(line, "s", 1), dil);
    g.Ho = field(line, "Ho", g.Ho); g.Wo = field(line, "Wo", g.Wo);
    return g;
}
static int run_cases() {
    static char line[1 << 14];
    while (fgets(line, sizeof(line), stdin)) {
        line[strcspn(line, "\r\n")] = 0;
        if (!line[0]) continue;
        emit("%s", line);
        if (!strncmp(line, "switches ", 9)) {
            set_switches(field(line, "sw", 0));
            flush_line();
        } else if (!strncmp(line, "conv ", 5)) {
            conv_call(line_geo(line, field(line, "d", 0)), field(line, "st", 0), field(line, "ad", 0), field(line, "bi", 0), field(line, "act", 0),
                      field(line, "om", 0), field(line, "oa", 0));
        } else if (!strncmp(line, "affine ", 7)) {
            affine_call(line_geo(line, 0), field(line, "re", 0), field(line, "sc", 1), field(line, "relu", 0), field(line, "oa", 0));
        } else if (!strncmp(line, "linear ", 7)) {
            linear_call(field(line, "M", 0), field(line, "N", 0), field(line, "K", 0), field(line, "maps", 0), field(line, "pg", 0), field(line, "act", 0),
                        field(line, "f32", 0), field(line, "re", 0), field(line, "rps", 0));
        } else if (!strncmp(line, "cgroup ", 7)) {
            PkConvDesc d[PK_GROUP_MAX + 1] = {};
            int n = 0;
            for (const char* c = line; (c = strstr(c, " m=")) && n <= PK_GROUP_MAX; c += 3, ++n) {
                int v[14] = {};
                sscanf(c + 3, "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11, v + 12, v + 13);
                PkConvDesc& m = d[n];
                m.x = fake<void>(X_, n << 20); m.w = fake<void>(W_, n << 20); m.out = fake<void>(OUT_, n << 20);
                m.B = v[0]; m.Hs = v[1]; m.Ws = v[2]; m.Cin = v[3]; m.Cout = v[4]; m.ksize = v[5]; m.stride = v[6]; m.dilated_input = v[7]; m.Ho = v[8]; m.Wo = v[9];
                m.stats = v[10] ? fake<float>(STATS_, n << 20) : nullptr;
                m.col_scale = v[11] ? fake<float>(SCALE_, n << 12) : nullptr;
                m.bias = v[11] ? fake<float>(BIAS_, n << 12) : nullptr;
                m.res = v[12] ? fake<void>(RES_, (n << 20) + (v[12] == 2 ? 8 : 0)) : nullptr;
                m.act = v[13];
            }
            finish(pk_conv2d_group(d, n, STREAM));
            flush_line();
        } else {
            emit(" | unknown line type");
            flush_line();
            return 2;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--cases")) return run_cases();
    sweep_conv();
    sweep_linear();
    sweep_wgrad();
    sweep_groups();
    return 0;
}
