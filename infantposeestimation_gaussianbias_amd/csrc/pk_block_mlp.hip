// Fused MLP half of the HRFormer block (A3, hrformer.py:262-293 + Mlp :38-64) for the high-resolution branches (C = 32 / 64).
//
//   MLP half:   y = x + s * ( fc2( gelu_erf( fc1( LayerNorm2(x) ) ) ) )            one launch, forward
//               backward = two launches that RECOMPUTE LayerNorm / fc1 / GELU from x:
//                 k_mlp_bwd_dx : dx (through fc2^T, GELU', fc1^T, LayerNorm backward, + the residual gradient), dgamma/dbeta slabs
//                 k_mlp_bwd_dw : dW1, db1, dW2, db2 slabs (hidden dimension sliced over blockIdx.y so the fp32 accumulators stay
//                                in registers)
//   The 4C-wide hidden activation never exists in HBM: per token the unfused chain moved 2C (v) + 2*8C (z, h) + ... bytes per
//   direction; here a forward launch reads x once and writes y once (4C bytes per token), the backward reads x, dy twice and
//   writes dx once.
// The operand layouts (accumulator order, fragment order) are described in pk_block.h.
#include "pk_block.h"

struct MlpArgs {
    const uint16_t* x;       // [M][C] bf16: input of the half (= residual)
    const uint16_t* dy;      // [M][C] bf16: gradient of the output (backward)
    uint16_t* out;           // forward: y; backward dx: dx
    const float *gamma, *beta, *b1, *b2;
    const float* scale;      // per-sample multiplier of the MLP branch (DropPath), or null
    const uint16_t* w1;      // fc1 weight  [4C][C]   (forward copy)
    const uint16_t* w2;      // fc2 weight  [C][4C]   (forward copy)
    const uint16_t* w1t;     // fc1 weight^T [C][4C]  (data-gradient copy)
    const uint16_t* w2t;     // fc2 weight^T [4C][C]  (data-gradient copy)
    float* part;             // backward: slabs (see the kernels)
    int M, rows_per_sample;
    float eps;
};

// ================================================================================================ forward
template <int C>
__global__ void __launch_bounds__(256) k_mlp_fwd(MlpArgs p) {
    constexpr int HD = 4 * C, NK = C / 32, NT = HD / 16, NS = HD / 32, NCT = C / 16, RT = 2;
    __shared__ __attribute__((aligned(16))) u32x4 sW1[NT * NK * 64];       // fragment (t, k): rows hid(t, i), channels 32k + 8g ..
    __shared__ __attribute__((aligned(16))) u32x4 sW2[NCT * NS * 64];      // fragment (ct, s): rows 16ct + i, hidden 32s + 8g ..
    __shared__ __attribute__((aligned(16))) float sB1[HD];
    const int tid = threadIdx.x, lane_ = tid & 63, wave = tid >> 6, i16 = lane_ & 15, g = lane_ >> 4;
    stage_frags(sW1, p.w1, NT * NK, C, [](int f, int i) { return hid(f / NK, i); }, [](int f) { return 32 * (f % NK); });
    stage_frags(sW2, p.w2, NCT * NS, HD, [](int f, int i) { return 16 * (f / NS) + i; }, [](int f) { return 32 * (f % NS); });
    for (int i = tid; i < HD; i += 256) sB1[i] = p.b1[i];
    LN_AFFINE_LOAD(gam, bet, NK, p.gamma, p.beta, g);
    f32x4 b2v[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) b2v[ct] = *reinterpret_cast<const f32x4*>(p.b2 + 16 * ct + 4 * g);
    __syncthreads();
    const auto rx = MAKE_RSRC(p.x);
    const auto ro = MAKE_RSRC(p.out);
    const int ngroups = (p.M + 16 * RT - 1) / (16 * RT);
    const float inv_c = 1.f / (float)C;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
        const int lane = opaque_lane<C != 32>(lane_);
        u32x4 xr[RT][NK];
        u32x2 xo[RT][NCT];
        unsigned rbase[RT];
        float sc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int row = grp * 16 * RT + 16 * rt + i16;
            const bool ok = row < p.M;
            rbase[rt] = ok ? (unsigned)row * (unsigned)(C * 2) : OOB_OFF;
#pragma unroll
            for (int k = 0; k < NK; ++k) xr[rt][k] = __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? rbase[rt] + (32 * k + 8 * g) * 2 : OOB_OFF, 0, 0);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) xo[rt][ct] = __builtin_amdgcn_raw_buffer_load_b64(rx, ok ? rbase[rt] + (16 * ct + 4 * g) * 2 : OOB_OFF, 0, 0);
            sc[rt] = (p.scale && ok) ? p.scale[row / p.rows_per_sample] : 1.f;
        }
        bf16x8 vf[RT][NK];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float mean, rstd;
            ln_row<NK>(xr[rt], gam, bet, inv_c, p.eps, vf[rt], mean, rstd);
        }
        f32x4 y[RT][NCT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) y[rt][ct] = zero;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            f32x4 h[RT][2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = 2 * s + u;
                const f32x4 bias = *reinterpret_cast<const f32x4*>(&sB1[32 * s + 8 * g + 4 * u]);     // b1[hid(t, 4g + r)]
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) h[rt][u] = bias;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const bf16x8 a = LDS_FRAG(sW1, t * NK + k, lane);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) h[rt][u] = MFMA(a, vf[rt][k], h[rt][u]);
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) h[rt][u] = gelu_erf(h[rt][u]);
            }
            bf16x8 hf[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) hf[rt] = pack2(h[rt][0], h[rt][1]);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const bf16x8 a = LDS_FRAG(sW2, ct * NS + s, lane);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) y[rt][ct] = MFMA(a, hf[rt], y[rt][ct]);
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const f32x4 o = (y[rt][ct] + b2v[ct]) * sc[rt] + unpack4(xo[rt][ct]);
                __builtin_amdgcn_raw_buffer_store_b64(pack4(o), ro, rbase[rt] == OOB_OFF ? OOB_OFF : rbase[rt] + (16 * ct + 4 * g) * 2, 0, 0);
            }
    }
}

// ================================================================================================ forward, wide channels
// C = 80 ... 320 (branches 2-3 of HRFormer-small, the 8-aligned twin of HRFormer-base): W1 and W2 (8 C^2 bytes each) do not fit the
// LDS any more, so the hidden dimension is walked in slices of 32 units and the 2 NK + NCT weight fragments of a slice (W1 rows of
// the slice, W2 columns of the slice) are STREAMED: global (L2-resident) -> registers -> a two-slot LDS ring in fragment order, the
// loads of slice s + 2 in flight while slice s is multiplied, one workgroup barrier per slice.  A workgroup is WAVES x 32 tokens
// (every wave reads every fragment: 8 waves = 256 tokens per 16 C^2 bytes of L2 traffic); x is read once for the LayerNorm / fc1
// operand and once more (L2 hit) for the residual, so the accumulators of fc2 (2 x NCT tiles) and the LayerNorm output (2 x NK
// fragments) are all a wave has to hold.  Channels beyond C inside the last 32-wide K step (C = 80: NK = 3) are zero operands: the
// loads of x, gamma, beta and of the weight columns are out of range there.  `c_real` < C (padded twins, models/padded.py): the
// LayerNorm statistics run over the real channels -- the padded ones hold exact zeros, so the sums only need the divisor, and the
// squared-deviation sum is corrected by (32 NK - c_real) mean^2.
// RESIDENT (C = 80 with hidden 320: 110 KB of fragments): every slice is staged ONCE per workgroup, the workgroups are persistent over
// 32-token groups and the waves run through the slices on their own -- no barrier after the prologue.
template <int NK, int NCT, int WAVES, bool RESIDENT>
__global__ void __launch_bounds__(64 * WAVES) k_mlp_fwd_w(MlpArgs p, int C, int c_real, int HD) {
    constexpr int RT = 2, NF = 2 * NK + NCT, NLD = (NF + WAVES - 1) / WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_w[];
    const int NS = HD >> 5, n_slots = RESIDENT ? NS : 2;
    u32x4* ring = reinterpret_cast<u32x4*>(smem_w);                      // [n_slots][NF][64] fragments
    float* sB1 = reinterpret_cast<float*>(smem_w + n_slots * NF * 1024); // [HD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const auto rw1 = MAKE_RSRC(p.w1), rw2 = MAKE_RSRC(p.w2);
    // staging: fragment f = wave + WAVES j of a slice is fetched by this wave (lane l = the fragment's lane)
    unsigned soff[NLD], sstep[NLD];
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
        const int f = wave + WAVES * j;
        if (f < 2 * NK) {                    // W1 rows hid(2s + u, i), columns 32k + 8g ..
            const int u = f / NK, k = f - u * NK, col = 32 * k + 8 * g;
            soff[j] = col < C ? (unsigned)((hid(u, i16) * C + col) * 2) : OOB_OFF;
            sstep[j] = 64u * (unsigned)C;
        } else if (f < NF) {                 // W2 rows 16ct + i, columns 32s + 8g ..
            const int ct = f - 2 * NK;
            soff[j] = (unsigned)(((16 * ct + i16) * HD + 8 * g) * 2);
            sstep[j] = 64u;
        } else {
            soff[j] = OOB_OFF;
            sstep[j] = 0u;
        }
    }
    u32x4 st[NLD];
    auto load_slice = [&](int s) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int f = wave + WAVES * j;
            st[j] = f < 2 * NK ? __builtin_amdgcn_raw_buffer_load_b128(rw1, soff[j] + sstep[j] * (unsigned)s, 0, 0)
                               : __builtin_amdgcn_raw_buffer_load_b128(rw2, soff[j] + sstep[j] * (unsigned)s, 0, 0);
        }
    };
    auto write_slice = [&](int slot) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int f = wave + WAVES * j;
            if (f < NF) ring[(slot * NF + f) * 64 + lane] = st[j];
        }
    };
    load_slice(0);
    for (int i = tid; i < HD; i += 64 * WAVES) sB1[i] = p.b1[i];
    if (RESIDENT) {
        for (int s = 0; s < NS; ++s) {
            write_slice(s);
            if (s + 1 < NS) load_slice(s + 1);
        }
        __syncthreads();
    }
    const auto rx = MAKE_RSRC(p.x);
    const auto ro = MAKE_RSRC(p.out);
    const auto rgam = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gamma), 0, C * 4, 0x00020000);
    const auto rbet = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.beta), 0, C * 4, 0x00020000);
    const auto rb2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.b2), 0, C * 4, 0x00020000);
    const float inv_c = 1.f / (float)c_real, n_pad = (float)(32 * NK - c_real);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int ngroups = (p.M + 16 * RT - 1) / (16 * RT);
    // (streamed: exactly one group per wave, grid = ceil(groups / WAVES), so every wave reaches every barrier; a group beyond the end is
    //  all out-of-range rows: zero loads, dropped stores)
    auto process = [&](const int grp) {
        // ---- this wave's 32 tokens: LayerNorm -> B-operand fragments
        unsigned rbase[RT];
        float sc[RT];
        bf16x8 vf[RT][NK];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int row = grp * 16 * RT + 16 * rt + i16;
            const bool ok = row < p.M;
            rbase[rt] = ok ? (unsigned)row * (unsigned)(C * 2) : OOB_OFF;
            sc[rt] = (p.scale && ok) ? p.scale[row / p.rows_per_sample] : 1.f;
            u32x4 xr[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) xr[k] = __builtin_amdgcn_raw_buffer_load_b128(rx, (ok && 32 * k + 8 * g < C) ? rbase[rt] + (32 * k + 8 * g) * 2 : OOB_OFF, 0, 0);
            float v[NK][8];
            float sm = 0.f;
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[k][2 * j] = blo(xr[k][j]);
                    v[k][2 * j + 1] = bhi(xr[k][j]);
                    sm += v[k][2 * j] + v[k][2 * j + 1];
                }
            sm = xor16_sum(sm);
            sm = xor32_sum(sm);
            const float mean = sm * inv_c;
            float q = 0.f;
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v[k][j] -= mean;
                    q += v[k][j] * v[k][j];
                }
            q = xor16_sum(q);
            q = xor32_sum(q);
            const float rstd = rsqrtf(fmaxf(q - n_pad * mean * mean, 0.f) * inv_c + p.eps);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const f32x4 g0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rgam, (32 * k + 8 * g) * 4, 0, 0));
                const f32x4 g1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rgam, (32 * k + 8 * g + 4) * 4, 0, 0));
                const f32x4 b0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rbet, (32 * k + 8 * g) * 4, 0, 0));
                const f32x4 b1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rbet, (32 * k + 8 * g + 4) * 4, 0, 0));
                u32x4 o;
                o[0] = pack_bf16x2(v[k][0] * rstd * g0[0] + b0[0], v[k][1] * rstd * g0[1] + b0[1]);
                o[1] = pack_bf16x2(v[k][2] * rstd * g0[2] + b0[2], v[k][3] * rstd * g0[3] + b0[3]);
                o[2] = pack_bf16x2(v[k][4] * rstd * g1[0] + b1[0], v[k][5] * rstd * g1[1] + b1[1]);
                o[3] = pack_bf16x2(v[k][6] * rstd * g1[2] + b1[2], v[k][7] * rstd * g1[3] + b1[3]);
                vf[rt][k] = __builtin_bit_cast(bf16x8, o);
            }
        }
        if (!RESIDENT) {
            write_slice(0);
            if (NS > 1) load_slice(1);
        }
        f32x4 y[RT][NCT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) y[rt][ct] = zero;
#pragma unroll 1
        for (int s = 0; s < NS; ++s) {
            if (!RESIDENT) {
                __syncthreads();          // slice s is visible to everyone, everyone is done with the other slot (slice s - 1)
                if (s + 1 < NS) write_slice((s + 1) & 1);
                if (s + 2 < NS) load_slice(s + 2);
            }
            const u32x4* fr = ring + (RESIDENT ? s : (s & 1)) * NF * 64;
            f32x4 h[RT][2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const f32x4 bias = *reinterpret_cast<const f32x4*>(&sB1[32 * s + 8 * g + 4 * u]);     // b1[hid(2s + u, 4g + r)]
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) h[rt][u] = bias;
            }
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bf16x8 a = LDS_FRAG(fr, u * NK + k, lane);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) h[rt][u] = MFMA(a, vf[rt][k], h[rt][u]);
                }
            bf16x8 hf[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                hf[rt] = pack2(gelu_erf_poly(h[rt][0]), gelu_erf_poly(h[rt][1]));          // packed-fp32 polynomial form (pk_common.h)
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const bf16x8 a = LDS_FRAG(fr, 2 * NK + ct, lane);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) y[rt][ct] = MFMA(a, hf[rt], y[rt][ct]);
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const unsigned off = rbase[rt] == OOB_OFF ? OOB_OFF : rbase[rt] + (16 * ct + 4 * g) * 2;
                const u32x2 xo = __builtin_amdgcn_raw_buffer_load_b64(rx, off, 0, 0);
                const f32x4 b2v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb2, (16 * ct + 4 * g) * 4, 0, 0));
                const f32x4 o = (y[rt][ct] + b2v) * sc[rt] + unpack4(xo);
                __builtin_amdgcn_raw_buffer_store_b64(pack4(o), ro, off, 0, 0);
            }
    };
    if (RESIDENT) {
        for (int grp = blockIdx.x * WAVES + wave; grp < ngroups; grp += gridDim.x * WAVES) process(grp);
    } else {
        process(blockIdx.x * WAVES + wave);
    }
}

// ================================================================================================ backward: dx
// dx = dy + LayerNorm_bwd( W1^T ( gelu'(z) * (W2^T (s dy)) ) ),  z = W1 LN(x) + b1 recomputed.  part[block][2][C] receives this
// workgroup's sums of dv * xhat (dgamma) and dv (dbeta), dv = gradient w.r.t. the LayerNorm output.
template <int C>
__global__ void __launch_bounds__(256) k_mlp_bwd_dx(MlpArgs p) {
    constexpr int HD = 4 * C, NK = C / 32, NT = HD / 16, NS = HD / 32, NCT = C / 16, RT = 2;
    __shared__ __attribute__((aligned(16))) u32x4 sW1[NT * NK * 64];       // (t, k): W1 rows hid(t, i), channels 32k + 8g ..
    __shared__ __attribute__((aligned(16))) u32x4 sW2T[NT * NK * 64];      // (t, k): W2^T rows hid(t, i), channels 32k + 8g ..
    __shared__ __attribute__((aligned(16))) u32x4 sW1T[NCT * NS * 64];     // (ct, s): W1^T rows 16ct + i, hidden 32s + 8g ..
    __shared__ __attribute__((aligned(16))) float sB1[HD];
    __shared__ float sRed[4][2][C];
    const int tid = threadIdx.x, lane_ = tid & 63, wave = tid >> 6, i16 = lane_ & 15, g = lane_ >> 4;
    stage_frags(sW1, p.w1, NT * NK, C, [](int f, int i) { return hid(f / NK, i); }, [](int f) { return 32 * (f % NK); });
    stage_frags(sW2T, p.w2t, NT * NK, C, [](int f, int i) { return hid(f / NK, i); }, [](int f) { return 32 * (f % NK); });
    stage_frags(sW1T, p.w1t, NCT * NS, HD, [](int f, int i) { return 16 * (f / NS) + i; }, [](int f) { return 32 * (f % NS); });
    for (int i = tid; i < HD; i += 256) sB1[i] = p.b1[i];
    LN_AFFINE_LOAD(gam, bet, NK, p.gamma, p.beta, g);
    f32x4 gamA[NCT], dgam[NCT], dbet[NCT];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        gamA[ct] = *reinterpret_cast<const f32x4*>(p.gamma + 16 * ct + 4 * g);
        dgam[ct] = dbet[ct] = zero;
    }
    __syncthreads();
    const auto rx = MAKE_RSRC(p.x);
    const auto rg = MAKE_RSRC(p.dy);
    const auto ro = MAKE_RSRC(p.out);
    const int ngroups = (p.M + 16 * RT - 1) / (16 * RT);
    const float inv_c = 1.f / (float)C;
    for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
        const int lane = opaque_lane<true>(lane_);
        u32x4 xr[RT][NK], dyr[RT][NK];
        u32x2 xo[RT][NCT], dyo[RT][NCT];
        unsigned rbase[RT];
        float sc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int row = grp * 16 * RT + 16 * rt + i16;
            const bool ok = row < p.M;
            rbase[rt] = ok ? (unsigned)row * (unsigned)(C * 2) : OOB_OFF;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const unsigned off = ok ? rbase[rt] + (32 * k + 8 * g) * 2 : OOB_OFF;
                xr[rt][k] = __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0);
                dyr[rt][k] = __builtin_amdgcn_raw_buffer_load_b128(rg, off, 0, 0);
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const unsigned off = ok ? rbase[rt] + (16 * ct + 4 * g) * 2 : OOB_OFF;
                xo[rt][ct] = __builtin_amdgcn_raw_buffer_load_b64(rx, off, 0, 0);
                dyo[rt][ct] = __builtin_amdgcn_raw_buffer_load_b64(rg, off, 0, 0);
            }
            sc[rt] = (p.scale && ok) ? p.scale[row / p.rows_per_sample] : 1.f;
        }
        bf16x8 vf[RT][NK], gf[RT][NK];
        float mean[RT], rstd[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            ln_row<NK>(xr[rt], gam, bet, inv_c, p.eps, vf[rt], mean[rt], rstd[rt]);
            scale_rows<NK>(dyr[rt], sc[rt], gf[rt]);
        }
        f32x4 dv[RT][NCT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) dv[rt][ct] = zero;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            f32x4 dz[RT][2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = 2 * s + u;
                const f32x4 bias = *reinterpret_cast<const f32x4*>(&sB1[32 * s + 8 * g + 4 * u]);
                f32x4 z[RT], dh[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    z[rt] = bias;
                    dh[rt] = zero;
                }
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const bf16x8 a1 = LDS_FRAG(sW1, t * NK + k, lane), a2 = LDS_FRAG(sW2T, t * NK + k, lane);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        z[rt] = MFMA(a1, vf[rt][k], z[rt]);
                        dh[rt] = MFMA(a2, gf[rt][k], dh[rt]);
                    }
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) dz[rt][u] = dh[rt] * gelu_grad(z[rt]);
            }
            bf16x8 dzf[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) dzf[rt] = pack2(dz[rt][0], dz[rt][1]);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const bf16x8 a = LDS_FRAG(sW1T, ct * NS + s, lane);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) dv[rt][ct] = MFMA(a, dzf[rt], dv[rt][ct]);
            }
        }
        // LayerNorm backward in accumulator layout: this lane holds channels 16ct + 4g + r of token (rt, i16)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            f32x4 xh[NCT];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                xh[ct] = (unpack4(xo[rt][ct]) - mean[rt]) * rstd[rt];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float gh = dv[rt][ct][r] * gamA[ct][r];
                    s1 += gh;
                    s2 += gh * xh[ct][r];
                }
                dgam[ct] += dv[rt][ct] * xh[ct];
                dbet[ct] += dv[rt][ct];
            }
            s1 = xor16_sum(s1);
            s1 = xor32_sum(s1);
            s2 = xor16_sum(s2);
            s2 = xor32_sum(s2);
            const float m1 = s1 * inv_c, m2 = s2 * inv_c;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const f32x4 o = (dv[rt][ct] * gamA[ct] - m1 - xh[ct] * m2) * rstd[rt] + unpack4(dyo[rt][ct]);
                __builtin_amdgcn_raw_buffer_store_b64(pack4(o), ro, rbase[rt] == OOB_OFF ? OOB_OFF : rbase[rt] + (16 * ct + 4 * g) * 2, 0, 0);
            }
        }
    }
    // dgamma / dbeta: tokens of this wave -> sum over the 16 lanes of a lane group, then over the 4 waves (fixed order)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a = dgam[ct][r], b = dbet[ct][r];
            a = lanes_sum<16>(a);
            b = lanes_sum<16>(b);
            if (i16 == 0) {
                sRed[wave][0][16 * ct + 4 * g + r] = a;
                sRed[wave][1][16 * ct + 4 * g + r] = b;
            }
        }
    __syncthreads();
    if (tid < 2 * C) {
        const int which = tid / C, c = tid - which * C;
        p.part[(size_t)blockIdx.x * 2 * C + tid] = ((sRed[0][which][c] + sRed[1][which][c]) + sRed[2][which][c]) + sRed[3][which][c];
    }
}

// ================================================================================================ backward: dW1, db1, dW2, db2
// blockIdx.y selects the hidden slice [h0, h0 + HS); slab of workgroup (x, y) at part + (y * gridDim.x + x) * SLAB:
//   [ dW1 slice [HS][C] | dW2 slice [C][HS] | db1 slice [HS] | db2 [C] ]   (fp32; db2 is the same in every slice: use slice 0)
template <int C, int HS>
__global__ void __launch_bounds__(256) k_mlp_bwd_dw(MlpArgs p) {
    constexpr int NK = C / 32, NTS = HS / 16, NSP = HS / 32, NCT = C / 16, RT = 2;
    constexpr int PV = C + 8, PH = 40;                               // row pitches (bf16) of the wave-private tiles
    constexpr int TILE_HALFS = 2 * 32 * PV + 2 * 32 * PH;            // v, g2, h, dz tiles of one wave
    constexpr int SLAB = 2 * HS * C + HS + C;
    constexpr int SCRATCH_BYTES = (4 * TILE_HALFS * 2 > SLAB * 4) ? 4 * TILE_HALFS * 2 : SLAB * 4;
    __shared__ __attribute__((aligned(16))) u32x4 sW1[NTS * NK * 64];      // (t, k): W1 rows h0 + 16t + i
    __shared__ __attribute__((aligned(16))) u32x4 sW2T[NTS * NK * 64];     // (t, k): W2^T rows h0 + 16t + i
    __shared__ __attribute__((aligned(16))) float sB1[HS];
    __shared__ __attribute__((aligned(16))) unsigned char sScratch[SCRATCH_BYTES];
    const int tid = threadIdx.x, lane_ = tid & 63, wave = tid >> 6, i16 = lane_ & 15, g = lane_ >> 4;
    const int h0 = blockIdx.y * HS;
    stage_frags(sW1, p.w1 + (size_t)h0 * C, NTS * NK, C, [](int f, int i) { return 16 * (f / NK) + i; }, [](int f) { return 32 * (f % NK); });
    stage_frags(sW2T, p.w2t + (size_t)h0 * C, NTS * NK, C, [](int f, int i) { return 16 * (f / NK) + i; }, [](int f) { return 32 * (f % NK); });
    for (int i = tid; i < HS; i += 256) sB1[i] = p.b1[h0 + i];
    uint16_t* tV = reinterpret_cast<uint16_t*>(sScratch) + wave * TILE_HALFS;
    uint16_t* tG = tV + 32 * PV;
    uint16_t* tH = tG + 32 * PV;
    uint16_t* tD = tH + 32 * PH;
    LN_AFFINE_LOAD(gam, bet, NK, p.gamma, p.beta, g);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dW1[NTS][NCT], dW2[NCT][NTS];
    float db1[NTS], db2[NCT];
#pragma unroll
    for (int t = 0; t < NTS; ++t) {
        db1[t] = 0.f;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) dW1[t][ct] = dW2[ct][t] = zero;
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) db2[ct] = 0.f;
    __syncthreads();
    const auto rx = MAKE_RSRC(p.x);
    const auto rg = MAKE_RSRC(p.dy);
    const int ngroups = (p.M + 16 * RT - 1) / (16 * RT);
    const float inv_c = 1.f / (float)C;
    for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
        const int lane = opaque_lane<true>(lane_);
        u32x4 xr[RT][NK], dyr[RT][NK];
        float sc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int row = grp * 16 * RT + 16 * rt + i16;
            const bool ok = row < p.M;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const unsigned off = ok ? (unsigned)row * (unsigned)(C * 2) + (32 * k + 8 * g) * 2 : OOB_OFF;
                xr[rt][k] = __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0);
                dyr[rt][k] = __builtin_amdgcn_raw_buffer_load_b128(rg, off, 0, 0);
            }
            sc[rt] = (p.scale && ok) ? p.scale[row / p.rows_per_sample] : 1.f;
        }
        bf16x8 vf[RT][NK], gf[RT][NK];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float mean, rstd;
            ln_row<NK>(xr[rt], gam, bet, inv_c, p.eps, vf[rt], mean, rstd);
            scale_rows<NK>(dyr[rt], sc[rt], gf[rt]);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                *reinterpret_cast<bf16x8*>(tV + (16 * rt + i16) * PV + 32 * k + 8 * g) = vf[rt][k];
                *reinterpret_cast<bf16x8*>(tG + (16 * rt + i16) * PV + 32 * k + 8 * g) = gf[rt][k];
            }
        }
        LDS_FENCE();
        bf16x8 vT[NCT], gT[NCT];          // lane = channel 16ct + i16, slots = the 32 tokens in accumulator order
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            vT[ct] = tr_frag32(tV, PV, 16 * ct, lane);
            gT[ct] = tr_frag32(tG, PV, 16 * ct, lane);
            db2[ct] += sum8(gT[ct]);
        }
#pragma unroll
        for (int sp = 0; sp < NSP; ++sp) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = 2 * sp + u;
                const f32x4 bias = *reinterpret_cast<const f32x4*>(&sB1[16 * t + 4 * g]);
                f32x4 z[RT], dh[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    z[rt] = bias;
                    dh[rt] = zero;
                }
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const bf16x8 a1 = LDS_FRAG(sW1, t * NK + k, lane), a2 = LDS_FRAG(sW2T, t * NK + k, lane);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        z[rt] = MFMA(a1, vf[rt][k], z[rt]);
                        dh[rt] = MFMA(a2, gf[rt][k], dh[rt]);
                    }
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    f32x4 hh, dz;                           // gelu and gelu' share the erf polynomial
                    gelu_both(z[rt], hh, dz);
                    dz *= dh[rt];
                    *reinterpret_cast<u32x2*>(tH + (16 * rt + i16) * PH + 16 * u + 4 * g) = pack4(hh);
                    *reinterpret_cast<u32x2*>(tD + (16 * rt + i16) * PH + 16 * u + 4 * g) = pack4(dz);
                }
            }
            LDS_FENCE();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = 2 * sp + u;
                const bf16x8 hT = tr_frag32(tH, PH, 16 * u, lane), dT = tr_frag32(tD, PH, 16 * u, lane);
                db1[t] += sum8(dT);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    dW2[ct][t] = MFMA(gT[ct], hT, dW2[ct][t]);      // D[c][hd] = sum_m g2[m][c] h[m][hd]
                    dW1[t][ct] = MFMA(dT, vT[ct], dW1[t][ct]);      // D[hd][c] = sum_m dz[m][hd] v[m][c]
                }
            }
            LDS_FENCE();                                             // the reads above complete before the tiles are rewritten
        }
    }
    // ---- the four waves' accumulators are summed in LDS in wave order (fixed order), then written as ONE slab per workgroup
    float* slab = reinterpret_cast<float*>(sScratch);
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < NTS; ++t) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* a = slab + (16 * t + 4 * g + r) * C + 16 * ct + i16;                 // dW1[hd][c]: lane = c, rows = hd
                        float* b = slab + HS * C + (16 * ct + 4 * g + r) * HS + 16 * t + i16;       // dW2[c][hd]: lane = hd, rows = c
                        *a = (w ? *a : 0.f) + dW1[t][ct][r];
                        *b = (w ? *b : 0.f) + dW2[ct][t][r];
                    }
                float v = db1[t];
                v = xor16_sum(v);
                v = xor32_sum(v);
                if (g == 0) {
                    float* a = slab + 2 * HS * C + 16 * t + i16;
                    *a = (w ? *a : 0.f) + v;
                }
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                float v = db2[ct];
                v = xor16_sum(v);
                v = xor32_sum(v);
                if (g == 0) {
                    float* a = slab + 2 * HS * C + HS + 16 * ct + i16;
                    *a = (w ? *a : 0.f) + v;
                }
            }
        }
    }
    __syncthreads();
    float* dst = p.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SLAB;
    for (int i = tid * 4; i < SLAB; i += 1024) *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(slab + i);
}

// ================================================================================================ C-ABI
static inline int mlp_hidden_slice(int C) {          // hidden units per blockIdx.y slice of the weight-gradient kernel
    // Measured (B = 64): the 128 accumulator registers of HS * C = 4096 hold the kernel at one wave per SIMD (C = 32: 66 us);
    // half of that (two waves per SIMD) runs the same work in 40 us although every slice recomputes LayerNorm.  (Round 4, with VGPR-form
    // MFMAs the 128-unit slice needs 255 registers, i.e. two waves per SIMD as well: 15.48-15.51 vs 15.43-15.51 ms per step -- no gain.)
    return C == 32 ? 64 : 32;
}
extern "C" int pk_ln_mlp_supported(int C) { return C == 32 || C == 64; }
extern "C" int pk_ln_mlp_hidden_slice(int C) { return mlp_hidden_slice(C); }
extern "C" int pk_ln_mlp_slab_floats(int C) {
    const int hs = mlp_hidden_slice(C);
    return 2 * hs * C + hs + C;
}
// workgroups (4 waves, one 32-token group per wave and iteration): enough to fill 256 CUs twice, never more than the work
static inline int mlp_blocks(int M, int target) { return capped_grid(((M + 31) / 32 + 3) / 4, target); }
constexpr int MLP_FWD_WGS = 512, MLP_DX_WGS = 512;          // forward and data gradient, C = 32 and C = 64 alike
static inline int mlp_dw_target(int C) {
    // (fewer, longer-lived workgroups: each one stages its weight slice and ends with a 4-phase slab reduction; 256 x slices
    // workgroups beat 512 and 1024 at every slice width; C = 64 with its 8 slices: 32 x 8 = one workgroup per CU; 64 x 8 = 38 us in
    // isolation and the step 0.07 ms slower (see attn_blocks, pk_block_attn.hip), 128 x 8 = 46 us, 256 x 8 = 67 us)
    return C == 32 ? 256 : 32;
}
extern "C" int pk_ln_mlp_dx_blocks(int M, int C) { return mlp_blocks(M, MLP_DX_WGS); }
extern "C" int pk_ln_mlp_dw_blocks(int M, int C) { return mlp_blocks(M, mlp_dw_target(C)); }
// Wide channels, forward only (inference; training of these widths takes the unfused sequence, whose backward needs the hidden saved).
// `M` > 0 also asks whether the launch pays: a workgroup walks ALL hidden slices for its 128 / 256 tokens, so a launch with few
// workgroups is one long serial chain per CU -- measured in cfg 5 (HRFormer-base twin, B = 64 with the flip): C = 320 with 13 824 tokens
// (108 workgroups) 151 us against ~70 us for the unfused fc1 + fc2 GEMMs (step 29.35 ms with it, 27.45 ms without), while C = 80
// (864 workgroups) and C = 160 (216) win 2.4 ms per step.  Hence at least min_wgs = 160 workgroups.
extern "C" int pk_ln_mlp_wide_supported(int C, int hidden, int M) {
    constexpr int min_wgs = 160;
    if (!((C == 80 || C == 128 || C == 160 || C == 256 || C == 320) && hidden > 0 && hidden % 32 == 0 && hidden <= 2048)) return 0;
    const int per_wg = C >= 256 ? 128 : 256;
    return M <= 0 || (M + per_wg - 1) / per_wg >= min_wgs;
}

// What every pk_ln_mlp_* entry passes on; the entry adds its own output, weights copies and slabs.
static MlpArgs mlp_args(const void* x, const float* gamma, const float* beta, const void* w1, const float* b1, const float* row_scale, int M,
                        int rows_per_sample, float eps) {
    MlpArgs a{};
    a.x = (const uint16_t*)x; a.gamma = gamma; a.beta = beta; a.b1 = b1; a.scale = row_scale; a.w1 = (const uint16_t*)w1;
    a.M = M; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; a.eps = eps;
    return a;
}
// The argument checks of every pk_ln_mlp_* entry, in the order they have always been made.  The wide forward differs in four places:
// what it is built for, it needs all its pointers at once and a sound `c_real`, it refuses a scale without rows_per_sample (the
// C = 32 / 64 entries have always taken rows_per_sample <= 0 as 1), its kernel walks hidden x C weights with 32-bit offsets and
// reads beta 16 bytes at a time.
struct MlpWide { int hidden, c_real, rows_per_sample; };
static int mlp_check(const char* who, const MlpArgs& a, int C, const MlpWide* wide = nullptr) {
    if (wide) PK_SUPPORTED(pk_ln_mlp_wide_supported(C, wide->hidden, 0), "%s: C=%d hidden=%d (built for C = 80 / 128 / 160 / 256 / 320, hidden %% 32 == 0)", who, C, wide->hidden);
    else PK_SUPPORTED(pk_ln_mlp_supported(C), "%s: C=%d (the fused MLP half is built for C = 32 / 64)", who, C);
    PK_REQUIRE(a.x && a.gamma && a.beta && a.b1 && (!wide || (a.w1 && a.w2 && a.b2 && a.out)) && a.M > 0, "%s: null pointer / bad size", who);
    if (wide) {
        PK_REQUIRE(wide->c_real > 0 && wide->c_real <= C, "%s: c_real=%d outside (0, C=%d]", who, wide->c_real, C);
        PK_REQUIRE(!a.scale || wide->rows_per_sample > 0, "%s: scale needs rows_per_sample", who);
    }
    PK_REQUIRE((int64_t)a.M * C < 0x3fffffffLL && (!wide || (int64_t)wide->hidden * C < 0x1fffffffLL), "%s: tensor too large for 32-bit byte offsets", who);
    PK_REQUIRE(((((uintptr_t)a.x) | ((uintptr_t)a.dy) | ((uintptr_t)a.out) | ((uintptr_t)a.w1) | ((uintptr_t)a.w2) | ((uintptr_t)a.w1t) |
                 ((uintptr_t)a.w2t) | ((uintptr_t)a.gamma) | ((uintptr_t)a.b2) | ((uintptr_t)a.part) | (wide ? (uintptr_t)a.beta : 0)) & 15) == 0,
               "%s: 16-byte alignment", who);
    return PK_OK;
}

extern "C" int pk_ln_mlp_fwd(const void* x, const float* gamma, const float* beta, const void* w1, const float* b1, const void* w2,
                             const float* b2, const float* row_scale, void* y, int M, int C, int rows_per_sample, float eps, void* stream) {
    MlpArgs a = mlp_args(x, gamma, beta, w1, b1, row_scale, M, rows_per_sample, eps);
    a.out = (uint16_t*)y; a.w2 = (const uint16_t*)w2; a.b2 = b2;
    int rc = mlp_check("pk_ln_mlp_fwd", a, C);
    if (rc) return rc;
    PK_REQUIRE(w1 && w2 && b2 && y, "pk_ln_mlp_fwd: null pointer");
    const dim3 grid(mlp_blocks(M, MLP_FWD_WGS)), block(256);
    if (C == 32) hipLaunchKernelGGL(k_mlp_fwd<32>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_mlp_fwd<64>, grid, block, 0, (hipStream_t)stream, a);
    return pk_launch_status("pk_ln_mlp_fwd");
}

template <int NK, int NCT, int WAVES>
static int mlp_wide_launch(const MlpArgs& a, int C, int c_real, int HD, hipStream_t st) {
    constexpr int NF = 2 * NK + NCT;
    const int NS = HD / 32, lds_res = NS * NF * 1024 + HD * 4;
    const bool resident = lds_res <= 150 * 1024;         // every slice fits: stage once, persistent workgroups, no per-slice barrier
    const int lds = resident ? lds_res : 2 * NF * 1024 + HD * 4;
    PK_RAISE_LDS_LIMIT_ONCE("pk_ln_mlp_wide_fwd", (k_mlp_fwd_w<NK, NCT, WAVES, true>), 150 * 1024);
    PK_RAISE_LDS_LIMIT_ONCE("pk_ln_mlp_wide_fwd", (k_mlp_fwd_w<NK, NCT, WAVES, false>), 2 * NF * 1024 + 2048 * 4);
    const int need = (a.M + 32 * WAVES - 1) / (32 * WAVES);
    if (resident) hipLaunchKernelGGL((k_mlp_fwd_w<NK, NCT, WAVES, true>), dim3(capped_grid(need, pk_cu_count())), dim3(64 * WAVES), lds, st, a, C, c_real, HD);
    else hipLaunchKernelGGL((k_mlp_fwd_w<NK, NCT, WAVES, false>), dim3(need), dim3(64 * WAVES), lds, st, a, C, c_real, HD);
    return pk_launch_status("pk_ln_mlp_wide_fwd");
}
extern "C" int pk_ln_mlp_wide_fwd(const void* x, const float* gamma, const float* beta, const void* w1, const float* b1, const void* w2,
                                  const float* b2, const float* row_scale, void* y, int M, int C, int c_real, int hidden,
                                  int rows_per_sample, float eps, void* stream) {
    MlpArgs a = mlp_args(x, gamma, beta, w1, b1, row_scale, M, rows_per_sample, eps);
    a.out = (uint16_t*)y; a.w2 = (const uint16_t*)w2; a.b2 = b2;
    const MlpWide wide{hidden, c_real, rows_per_sample};
    int rc = mlp_check("pk_ln_mlp_wide_fwd", a, C, &wide);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 80: return mlp_wide_launch<3, 5, 8>(a, C, c_real, hidden, st);
        case 128: return mlp_wide_launch<4, 8, 8>(a, C, c_real, hidden, st);
        case 160: return mlp_wide_launch<5, 10, 8>(a, C, c_real, hidden, st);
        case 256: return mlp_wide_launch<8, 16, 4>(a, C, c_real, hidden, st);
        default: return mlp_wide_launch<10, 20, 4>(a, C, c_real, hidden, st);
    }
}

extern "C" int pk_ln_mlp_bwd_dx(const void* dy, const void* x, const float* gamma, const float* beta, const void* w1, const float* b1,
                                const void* w1_t, const void* w2_t, const float* row_scale, void* dx, float* ln_partial, int M, int C,
                                int rows_per_sample, float eps, void* stream) {
    MlpArgs a = mlp_args(x, gamma, beta, w1, b1, row_scale, M, rows_per_sample, eps);
    a.dy = (const uint16_t*)dy; a.out = (uint16_t*)dx; a.w1t = (const uint16_t*)w1_t; a.w2t = (const uint16_t*)w2_t; a.part = ln_partial;
    int rc = mlp_check("pk_ln_mlp_bwd_dx", a, C);
    if (rc) return rc;
    PK_REQUIRE(dy && w1 && w1_t && w2_t && dx && ln_partial, "pk_ln_mlp_bwd_dx: null pointer");
    const dim3 grid(pk_ln_mlp_dx_blocks(M, C)), block(256);
    if (C == 32) hipLaunchKernelGGL(k_mlp_bwd_dx<32>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_mlp_bwd_dx<64>, grid, block, 0, (hipStream_t)stream, a);
    return pk_launch_status("pk_ln_mlp_bwd_dx");
}

extern "C" int pk_ln_mlp_bwd_dw(const void* dy, const void* x, const float* gamma, const float* beta, const void* w1, const float* b1,
                                const void* w2_t, const float* row_scale, float* slabs, int M, int C, int rows_per_sample, float eps,
                                void* stream) {
    MlpArgs a = mlp_args(x, gamma, beta, w1, b1, row_scale, M, rows_per_sample, eps);
    a.dy = (const uint16_t*)dy; a.w2t = (const uint16_t*)w2_t; a.part = slabs;
    int rc = mlp_check("pk_ln_mlp_bwd_dw", a, C);
    if (rc) return rc;
    PK_REQUIRE(dy && w1 && w2_t && slabs, "pk_ln_mlp_bwd_dw: null pointer");
    const int hs = mlp_hidden_slice(C);
    const dim3 grid(pk_ln_mlp_dw_blocks(M, C), (4 * C) / hs), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (C == 32) hipLaunchKernelGGL((k_mlp_bwd_dw<32, 64>), grid, block, 0, st, a);          // <C, mlp_hidden_slice(C)>
    else hipLaunchKernelGGL((k_mlp_bwd_dw<64, 32>), grid, block, 0, st, a);
    return pk_launch_status("pk_ln_mlp_bwd_dw");
}
