// hpa_gemm_fp4w.hip -- the fused layer GEMMs on MXFP4 weights (OCP
// microscaling: e2m1 codes, one e8m0 power-of-two scale per 32 consecutive k
// of a row), weight-only (W4A16).  Two kernels, siblings of the fp8-weight
// looped kernel (hpa_gemm_fp8w.hip) and of the bf16 A-resident kernel
// (hpa_gemm_bf16.hip): the same launches, epilogues, XCD-aware grid, MFMA
// (v_mfma_f32_16x16x32_bf16, fp32 accumulation) and A operand (LN'ed fp32
// frag activations rounded to bf16), with the weights streamed at 4.25 bits
// per element and decoded to bf16 in registers by gfx950's
// v_cvt_scalef32_pk_bf16_fp4, which takes the group scale as an operand.
//
// Numerics: for row n and group g (k in [32g, 32g + 32)): t = the smallest
// integer with absmax / 2^t <= 6, clamped to [-64, 64], 0 for an all-zero
// group, stored as the e8m0 byte t + 127; code = e2m1_rne(clamp(w 2^-t, -6,
// 6)), ties to the even mantissa, bit 3 the sign.  decode(code) 2^t is exactly
// a bf16 value and is what the convert returns: the scale is applied at
// decode, nothing is multiplied after the fold, and the result is what the
// bf16-weight numerics give on W' = decode(code) 2^t.
//
// fp4 frag layout of a [rows][K] matrix (rows padded to 16, K % 64 == 0): the
// unit is (16-row block, 64-deep step s), 512 B contiguous, 8 bytes per lane.
// Lane l = (row l & 15, group g = l >> 4); its dword h (0, 1) holds, low
// nibble first, the codes of k = 64s + 32h + {4g..4g+3, 16+4g..16+4g+3}: the
// eight k of the two float4 the same lane loads from the fp32 frag layout at
// k16-steps 4s + 2h and 4s + 2h + 1.  Four converts (one per byte) turn dword
// h into the B fragment of the unit's MFMA k-step h; the A fragment is the
// bf16 pack of that float4 pair.  Each MFMA k-step is one MX group per row, so
// a lane needs one scale byte per (row, k-step): the two bytes of (row, s) sit
// together in unit order, [row block][s][16 rows][2], 32 B per unit, and the
// float scale is (unsigned)byte << 23.
#include <math.h>

#include "hpa_gemm_body.h"
#include "hpa_mx_quant.h"

namespace hpa_gemm {

typedef __bf16 f4w_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned f4w_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short f4w_u16x8 __attribute__((ext_vector_type(8)));

// two e2m1 codes (byte B of a dword) -> two bf16 in one dword, times the
// group scale, exact.  The portable route (other targets, the host pass)
// takes the magnitudes from a table and the high halves of the products.
template <int B>
__device__ __forceinline__ unsigned e2m1x2_to_bf16(unsigned w, float scale) {
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4)
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, B));
#else
    const unsigned c = (w >> (8 * B)) & 0xffu;
    unsigned r = 0;
    for (int i = 0; i < 2; ++i) {
        const unsigned n = (c >> (4 * i)) & 0xfu, m = n & 7u;
        const float v = (m < 4 ? 0.5f * (float)m : m == 4 ? 2.f : m == 5 ? 3.f : m == 6 ? 4.f : 6.f) * scale;
        r |= ((__float_as_uint(v) >> 16) | ((n & 8u) << 12)) << (16 * i);
    }
    return r;
#endif
}
// one dword of codes and its group's scale byte -> the B fragment of an MFMA k-step
__device__ __forceinline__ f4w_bf16x8 f4w_frag(unsigned c, unsigned scale_byte) {
    const float s = __uint_as_float(scale_byte << 23);
    f4w_u32x4 u;
    u[0] = e2m1x2_to_bf16<0>(c, s);
    u[1] = e2m1x2_to_bf16<1>(c, s);
    u[2] = e2m1x2_to_bf16<2>(c, s);
    u[3] = e2m1x2_to_bf16<3>(c, s);
    return __builtin_bit_cast(f4w_bf16x8, u);
}
__device__ __forceinline__ f4w_bf16x8 f4w_pack_a(float4 a, float4 b) {
    f4w_u16x8 u;
    u[0] = hpa::f32_to_bf16(a.x);
    u[1] = hpa::f32_to_bf16(a.y);
    u[2] = hpa::f32_to_bf16(a.z);
    u[3] = hpa::f32_to_bf16(a.w);
    u[4] = hpa::f32_to_bf16(b.x);
    u[5] = hpa::f32_to_bf16(b.y);
    u[6] = hpa::f32_to_bf16(b.z);
    u[7] = hpa::f32_to_bf16(b.w);
    return __builtin_bit_cast(f4w_bf16x8, u);
}

// ---- looped kernel (variant 1).  The activations size the trip: U 64-deep
// steps of them per buffer, two buffers, as the fp8 kernel (16 * MT registers
// a step).  A step of weights is 2 * NTW registers, half the fp8 kernel's, so
// a WEIGHT trip is two activation trips: a weight buffer holds 2U steps, is
// loaded a whole weight trip ahead, and the two activation buffers alternate
// under it.  Weight registers and weight bytes in flight per wave equal the
// fp8 kernel's (2 buffers x 2U steps x NTW x 512 B); the scales add one
// register per (step, tile).
template <int MT, int NTW>
constexpr int f4w_trip() {
    return (4 * MT + NTW) <= 5 ? 2 : 1;
}

// MT = 16-row blocks, NTW = 16-column tiles per workgroup, NW = waves sharing
// the K range in contiguous runs of 64-deep steps (wave w: steps [w * per,
// w * per + per) with per = ceil(K/64 / NW), folded in wave order; a wave past
// the end folds zeros): a row's summation order depends on NW only.
template <int NW, int EPI, int MT, int NTW>
__global__ __launch_bounds__(NW * 64) void gemm_f4w_kernel(FG p, const unsigned short* __restrict__ gscale) {
    constexpr int U = f4w_trip<MT, NTW>();
    using E = Epi<NW, EPI, MT, NTW>;
    __shared__ __attribute__((aligned(16))) float smem[gemm16_lds_floats<NW, MT, NTW>()];
    constexpr int R = MT * 16;
    float* lngb = smem;                         // LN weight [K], bias [K]
    float* red = smem + 2 * HPA_FUSED_LN_KMAX;  // [NW][NTW][MT x 4][64]
    float* tile = red + NW * MT * NTW * 256;    // [NTW][R][17]
    float* lnst = tile + NTW * R * 17;          // [R][2]
    float* lnscr = lnst + 2 * R;                // [4R][2]

    int cx, ry;
    if (!xcd_tile(p, blockIdx.x, cx, ry)) return;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: scalar step bounds
    const int nt0 = cx * NTW;
    const int row0 = ry * MT * 16;
    const int q4 = lane >> 4;

    const int K64 = p.K >> 6;
    const int per = (K64 + NW - 1) / NW;
    const int kb0 = w * per;
    const int nsteps = max(0, min(K64, kb0 + per) - kb0);
    const uint2* __restrict__ wf[NTW];
    const unsigned short* __restrict__ sf[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {  // tail tiles past ntn re-read the last tile (never stored)
        const size_t t = (size_t)min(nt0 + j, p.ntn - 1) * K64;
        wf[j] = reinterpret_cast<const uint2*>(p.w) + t * 64 + lane;
        sf[j] = gscale + t * 16 + (lane & 15);
    }
    const float4* __restrict__ xf = reinterpret_cast<const float4*>(p.x) + (size_t)ry * MT * p.K16 * 64 + lane;
    const size_t rbs = (size_t)p.K16 * 64;  // float4 stride between row blocks
    const bool ln_apply = p.ln_stats != nullptr;
    const float4* sg = reinterpret_cast<const float4*>(lngb) + q4;
    const float4* sb = reinterpret_cast<const float4*>(lngb + HPA_FUSED_LN_KMAX) + q4;

    struct WBuf {  // a weight trip: 2U steps
        uint2 c[2 * U][NTW];
        unsigned s[2 * U][NTW];
    };
    struct XBuf {  // an activation trip: U steps
        float4 x[U][MT][4];
    };
    WBuf WA, WB;
    XBuf XA, XB;
    // clamped, unconditional loads (callers: nsteps > 0): a step past the
    // wave's end re-reads its last step and comp skips it
    auto load_w = [&](WBuf& f, int T) {
#pragma unroll
        for (int u = 0; u < 2 * U; ++u) {
            const int k = kb0 + min(T * 2 * U + u, nsteps - 1);
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                f.c[u][j] = wf[j][(size_t)k * 64];
                f.s[u][j] = sf[j][(size_t)k * 16];
            }
        }
    };
    auto load_x = [&](XBuf& f, int t) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kb0 + min(t * U + u, nsteps - 1);
#pragma unroll
            for (int r = 0; r < MT; ++r)
#pragma unroll
                for (int d = 0; d < 4; ++d) f.x[u][r][d] = xf[r * rbs + (size_t)(4 * k + d) * 64];
        }
    };
    const int wtrips = (nsteps + 2 * U - 1) / (2 * U);
    if (wtrips > 0) {  // first operands in flight during the LN prologue
        load_w(WA, 0);
        load_x(XA, 0);
    }

    float mu[MT], rs[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) mu[r] = rs[r] = 0.f;
    if (ln_apply) ln_prologue<NW, MT>(p, lngb, lnst, lnscr, row0, true, mu, rs);

    f32x4 acc[MT * NTW];
#pragma unroll
    for (int i = 0; i < MT * NTW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // activation trip t on half hh of weight trip t / 2
    auto comp = [&](WBuf& fw, int hh, XBuf& fx, int t) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t * U + u < nsteps) {
                const int k = kb0 + t * U + u;
#pragma unroll
                for (int h = 0; h < 2; ++h) {  // the unit's two MFMA k-steps, one MX group each
                    f4w_bf16x8 xa[MT];
                    float4 g0, b0, g1, b1;
                    if (ln_apply) {
                        g0 = sg[4 * (4 * k + 2 * h)];
                        b0 = sb[4 * (4 * k + 2 * h)];
                        g1 = sg[4 * (4 * k + 2 * h + 1)];
                        b1 = sb[4 * (4 * k + 2 * h + 1)];
                    }
#pragma unroll
                    for (int r = 0; r < MT; ++r) {
                        float4 x0 = fx.x[u][r][2 * h], x1 = fx.x[u][r][2 * h + 1];
                        if (ln_apply) {
                            x0 = ln4(x0, mu[r], rs[r], g0, b0);
                            x1 = ln4(x1, mu[r], rs[r], g1, b1);
                        }
                        xa[r] = f4w_pack_a(x0, x1);
                    }
#pragma unroll
                    for (int j = 0; j < NTW; ++j) {  // decoded once, used by all MT row blocks
                        const uint2 c = fw.c[hh * U + u][j];
                        const unsigned s = fw.s[hh * U + u][j];
                        const f4w_bf16x8 wb = h == 0 ? f4w_frag(c.x, s & 0xffu) : f4w_frag(c.y, s >> 8);
#pragma unroll
                        for (int r = 0; r < MT; ++r)
                            acc[j * MT + r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[r], wb, acc[j * MT + r], 0, 0, 0);
                    }
                }
            }
        }
    };
    // no exit between the halves, as gemm_f8w_kernel
    for (int T = 0; T < wtrips; T += 2) {
        load_w(WB, T + 1);
        load_x(XB, 2 * T + 1);
        comp(WA, 0, XA, 2 * T);
        load_x(XA, 2 * T + 2);
        comp(WA, 1, XB, 2 * T + 1);
        load_w(WA, T + 2);
        load_x(XB, 2 * T + 3);
        comp(WB, 0, XA, 2 * T + 2);
        load_x(XA, 2 * T + 4);
        comp(WB, 1, XB, 2 * T + 3);
    }

    // the shared fold (wave order), then the shared epilogue: no scale here
    E epi;
    epi.prefetch(p, nt0, row0);
    float vals[E::EPT];
    E::fold(acc, red, vals);
    epi.apply(p, vals, tile, nt0, row0, nullptr);
}

template <int NW, int MT, int NTW>
static int launch_f4w_t(FG p, const unsigned short* gs, int epi) {
    const int gx = (p.ntn + NTW - 1) / NTW, gy = p.Mp / 16 / MT;
    p.gx = gx;
    p.gy = gy;
    dim3 grid((unsigned)(((gx + 7) / 8) * 8 * gy)), block(NW * 64);
    switch (epi) {
        case HPA_FEPI_QKV: gemm_f4w_kernel<NW, HPA_FEPI_QKV, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, gs); break;
        case HPA_FEPI_RESID: gemm_f4w_kernel<NW, HPA_FEPI_RESID, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, gs); break;
        case HPA_FEPI_GELU: gemm_f4w_kernel<NW, HPA_FEPI_GELU, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, gs); break;
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused fp4 weights: epilogue QKV, RESID or GELU");
    }
    HPA_LAUNCH_CHECK();
    return 0;
}

template <int NW>
static int launch_f4w_nw(const FG& p, const unsigned short* gs, int epi, int mt, int ntw) {
    switch (mt * 10 + ntw) {
        case 11: return launch_f4w_t<NW, 1, 1>(p, gs, epi);
        case 21: return launch_f4w_t<NW, 2, 1>(p, gs, epi);
        case 41: return launch_f4w_t<NW, 4, 1>(p, gs, epi);
        case 22: return launch_f4w_t<NW, 2, 2>(p, gs, epi);
        case 42: return launch_f4w_t<NW, 4, 2>(p, gs, epi);
        default:
            return hpa_fail(__FILE__, __LINE__,
                            "gemm_fused fp4 weights: (row_blocks, col_tiles) in {(1,1), (2,1), (4,1), (2,2), (4,2)}");
    }
}

int launch_f4w(const FG& p, const unsigned char* gscale, int epi, int nw, int mt, int ntw) {
    const unsigned short* gs = reinterpret_cast<const unsigned short*>(gscale);
    switch (nw) {
        case 4: return launch_f4w_nw<4>(p, gs, epi, mt, ntw);
        case 8: return launch_f4w_nw<8>(p, gs, epi, mt, ntw);
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused fp4 weights: waves must be 4 or 8");
    }
}

// ---- A-resident kernel (variant 5), after gemm_b16_ares_kernel: the
// workgroup's MT*16 rows of A are LayerNorm'ed and rounded to bf16 ONCE into
// LDS (bf16 frag layout: one bf16x8 per lane and 32-deep step), then wave w
// walks column tile c0 + round*NW + w over the whole K: it streams the tile's
// code dwordx2 and scale halfwords U 64-deep steps ahead, decodes in
// registers and reads the A fragments from LDS.  No K split and no fold: a
// row's sum is one in-order k chain, the same for every launch shape of this
// variant.  KC = A capacity in 32-deep steps (24: K <= 768, 50: 1600, 100:
// 3200), MT * KC <= 100.  U = 12: a K = 768 tile is one trip, 6 KiB a wave in
// flight at 36 registers.
template <int NW, int MT>
constexpr int f4w_ares_union_floats() {
    constexpr int red = NW * MT * 256 > NW * MT * 16 * 17 ? NW * MT * 256 : NW * MT * 16 * 17;
    return red > 2 * HPA_FUSED_LN_KMAX ? red : 2 * HPA_FUSED_LN_KMAX;
}
template <int NW, int MT, int KC>
constexpr int f4w_ares_lds_floats() {
    return f4w_ares_union_floats<NW, MT>() + 10 * MT * 16 + MT * KC * 64 * 4;
}

template <int NW, int EPI, int MT, int KC, int U>
__global__ __launch_bounds__(NW * 64) void gemm_f4w_ares_kernel(FG p, const unsigned short* __restrict__ gscale, int cpw) {
    constexpr int NT = NW * 64;
    constexpr int R = MT * 16;
    constexpr int TE = MT * 256;
    constexpr int EPT = TE / 64;  // elements per thread of one round (NW tiles x TE over NT)
    __shared__ __attribute__((aligned(16))) float smem[f4w_ares_lds_floats<NW, MT, KC>()];
    float* lngb = smem;                                    // LN weight [K], bias [K] (staging only)
    float* red = smem;                                     // [NW][TE] tile scratch (rounds only)
    float* lnst = smem + f4w_ares_union_floats<NW, MT>();  // [R][2]
    float* lnscr = lnst + 2 * R;                           // [4R][2]
    uint4* As = reinterpret_cast<uint4*>(lnscr + 8 * R);   // [MT][K32][64 lanes] bf16x8

    int cx, ry;
    if (!xcd_tile(p, blockIdx.x, cx, ry)) return;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int row0 = ry * R;
    const int K32 = p.K >> 5, K64 = p.K >> 6;
    const int t_begin = cx * cpw, t_end = min(p.ntn, t_begin + cpw);

    // 1. A: LN'ed, rounded, into LDS
    const bool ln_apply = p.ln_stats != nullptr;
    float mu[MT], rs[MT];
    if (ln_apply) ln_prologue<NW, MT>(p, lngb, lnst, lnscr, row0, true, mu, rs);
    {
        const float4* xf = reinterpret_cast<const float4*>(p.x) + (size_t)ry * MT * p.K16 * 64 + lane;
        const float4* sg = reinterpret_cast<const float4*>(lngb) + (lane >> 4);
        const float4* sb = reinterpret_cast<const float4*>(lngb + HPA_FUSED_LN_KMAX) + (lane >> 4);
        const int nst = MT * K32;
        for (int i = w; i < nst; i += NW) {  // (row block, 32-deep step) pairs, one per wave
            const int r = i / K32, st = i - r * K32;
            float4 x0 = xf[(size_t)r * p.K16 * 64 + (size_t)(2 * st) * 64];
            float4 x1 = xf[(size_t)r * p.K16 * 64 + (size_t)(2 * st + 1) * 64];
            if (ln_apply) {
                const float m = lnst[2 * (16 * r + (lane & 15))], q = lnst[2 * (16 * r + (lane & 15)) + 1];
                x0 = ln4(x0, m, q, sg[4 * (2 * st)], sb[4 * (2 * st)]);
                x1 = ln4(x1, m, q, sg[4 * (2 * st + 1)], sb[4 * (2 * st + 1)]);
            }
            As[(size_t)(r * K32 + st) * 64 + lane] = __builtin_bit_cast(uint4, f4w_pack_a(x0, x1));
        }
    }
    __syncthreads();

    // 2. rounds of NW column tiles
    for (int tb = t_begin; tb < t_end; tb += NW) {
        Epi<NW, EPI, MT, NW> epi;
        epi.prefetch(p, tb, row0);
        const int t = min(tb + w, p.ntn - 1);  // past the chunk: computed, never stored (col >= N or next round)
        const uint2* wp = reinterpret_cast<const uint2*>(p.w) + (size_t)t * K64 * 64 + lane;
        const unsigned short* sp = gscale + (size_t)t * K64 * 16 + (lane & 15);
        f32x4 acc[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        uint2 wq[U];
        unsigned sq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            wq[u] = wp[(size_t)min(u, K64 - 1) * 64];
            sq[u] = sp[(size_t)min(u, K64 - 1) * 16];
        }
        for (int s0 = 0; s0 < K64; s0 += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int st = s0 + u;
                const uint2 wc = wq[u];
                const unsigned sc = sq[u];
                wq[u] = wp[(size_t)min(st + U, K64 - 1) * 64];  // U steps ahead, clamped (unconditional)
                sq[u] = sp[(size_t)min(st + U, K64 - 1) * 16];
                if (st < K64) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f4w_bf16x8 wb = h == 0 ? f4w_frag(wc.x, sc & 0xffu) : f4w_frag(wc.y, sc >> 8);
#pragma unroll
                        for (int r = 0; r < MT; ++r) {
                            const f4w_bf16x8 a = __builtin_bit_cast(f4w_bf16x8, As[(size_t)(r * K32 + 2 * st + h) * 64 + lane]);
                            acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wb, acc[r], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // wave w's tile is column tile j = w of the round's Epi<.., NTW = NW>
#pragma unroll
        for (int r = 0; r < MT; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) red[w * TE + (r * 4 + g) * 64 + lane] = acc[r][g];
        __syncthreads();
        float vals[EPT];
#pragma unroll
        for (int i = 0; i < EPT; ++i) vals[i] = red[threadIdx.x + i * NT];
        __syncthreads();  // tile (the row statistics' scratch) aliases red
        epi.apply(p, vals, red, tb, row0, nullptr);
        __syncthreads();
    }
}

template <int NW, int MT, int KC>
static int launch_f4w_ares_t(FG p, const unsigned short* gs, int epi, int rounds) {
    constexpr int U = 12;
    const int gy = p.Mp / 16 / MT;
    if (rounds <= 0) {  // auto: one pass of workgroups over the CUs at this LDS footprint
        constexpr int lds = f4w_ares_lds_floats<NW, MT, KC>() * 4;
        const int per_cu = (160 * 1024) / lds > 0 ? (160 * 1024) / lds : 1;
        const int slots = 256 * per_cu;
        rounds = (p.ntn * gy + NW * slots - 1) / (NW * slots);
        if (rounds < 1) rounds = 1;
    }
    const int cpw = NW * rounds;
    const int gx = (p.ntn + cpw - 1) / cpw;
    p.gx = gx;
    p.gy = gy;
    dim3 grid((unsigned)(((gx + 7) / 8) * 8 * gy)), block(NW * 64);
    switch (epi) {
        case HPA_FEPI_QKV: gemm_f4w_ares_kernel<NW, HPA_FEPI_QKV, MT, KC, U><<<grid, block, 0, hpa_stream()>>>(p, gs, cpw); break;
        case HPA_FEPI_RESID: gemm_f4w_ares_kernel<NW, HPA_FEPI_RESID, MT, KC, U><<<grid, block, 0, hpa_stream()>>>(p, gs, cpw); break;
        case HPA_FEPI_GELU: gemm_f4w_ares_kernel<NW, HPA_FEPI_GELU, MT, KC, U><<<grid, block, 0, hpa_stream()>>>(p, gs, cpw); break;
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused fp4 weights: epilogue QKV, RESID or GELU");
    }
    HPA_LAUNCH_CHECK();
    return 0;
}

int launch_f4w_ares(const FG& p, const unsigned char* gscale, int epi, int nw, int mt, int rounds) {
    const unsigned short* gs = reinterpret_cast<const unsigned short*>(gscale);
    HPA_REQUIRE(rounds >= 0 && (p.Mp / 16) % mt == 0, "gemm_fused fp4 A-resident: rounds >= 0 (0: auto), row blocks of M");
    HPA_REQUIRE((mt == 4 && p.K <= 768) || (mt == 2 && p.K <= 1600) || (mt == 1 && p.K <= 3200),
                "gemm_fused fp4 A-resident: row_blocks * K <= 3200 (4: K <= 768, 2: 1600, 1: 3200)");
    const int k32 = p.K / 32;
    const int kc = k32 <= 24 ? 24 : k32 <= 50 ? 50 : 100;
    switch (nw * 1000 + mt * 100 + kc) {  // kc in {24, 50, 100}: keys unique
        case 4424: return launch_f4w_ares_t<4, 4, 24>(p, gs, epi, rounds);
        case 4224: return launch_f4w_ares_t<4, 2, 24>(p, gs, epi, rounds);
        case 4250: return launch_f4w_ares_t<4, 2, 50>(p, gs, epi, rounds);
        case 4124: return launch_f4w_ares_t<4, 1, 24>(p, gs, epi, rounds);
        case 4150: return launch_f4w_ares_t<4, 1, 50>(p, gs, epi, rounds);
        case 4200: return launch_f4w_ares_t<4, 1, 100>(p, gs, epi, rounds);  // mt 1, kc 100
        case 8424: return launch_f4w_ares_t<8, 4, 24>(p, gs, epi, rounds);
        case 8224: return launch_f4w_ares_t<8, 2, 24>(p, gs, epi, rounds);
        case 8250: return launch_f4w_ares_t<8, 2, 50>(p, gs, epi, rounds);
        case 8124: return launch_f4w_ares_t<8, 1, 24>(p, gs, epi, rounds);
        case 8150: return launch_f4w_ares_t<8, 1, 50>(p, gs, epi, rounds);
        case 8200: return launch_f4w_ares_t<8, 1, 100>(p, gs, epi, rounds);
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused fp4 A-resident: waves 4/8, row_blocks 1/2/4");
    }
}

}  // namespace hpa_gemm

namespace {
__device__ __forceinline__ unsigned f4w_code8(float4 a, float4 b, float inv) {
    return f4w_code(a.x, inv) | f4w_code(a.y, inv) << 4 | f4w_code(a.z, inv) << 8 | f4w_code(a.w, inv) << 12 |
           f4w_code(b.x, inv) << 16 | f4w_code(b.y, inv) << 20 | f4w_code(b.z, inv) << 24 | f4w_code(b.w, inv) << 28;
}
__device__ __forceinline__ float f4w_absmax8(float4 a, float4 b) {
    return fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))),
                 fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
}

// one 256-thread workgroup per 16-row block; each wave takes units s = wave,
// wave + 4, ...: lane (row, g) loads its sixteen elements of the unit, the four
// lanes of a row reduce each k-step's group absmax (a maximum: the same in any
// order), and the lane writes its 8 bytes of codes; g = 0 writes the row's two
// scale bytes.  Padded rows: code 0, scale byte 127.
__global__ __launch_bounds__(256) void pack_frag_fp4_kernel(const float* __restrict__ src, int rows, int K, int ld,
                                                            uint2* __restrict__ dst, unsigned short* __restrict__ scales) {
    const int rb = blockIdx.x;
    const int K64 = K >> 6;
    const int lane = threadIdx.x & 63;
    const int m = rb * 16 + (lane & 15);
    for (int s = threadIdx.x >> 6; s < K64; s += 4) {
        float4 v[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) v[d] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < rows) {
            const float* row = src + (size_t)m * ld + 64 * s + 4 * (lane >> 4);
#pragma unroll
            for (int d = 0; d < 4; ++d) v[d] = *reinterpret_cast<const float4*>(row + 16 * d);
        }
        uint2 c;
        unsigned sb = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float a = f4w_absmax8(v[2 * h], v[2 * h + 1]);
            a = fmaxf(a, __shfl_xor(a, 16, 64));
            a = fmaxf(a, __shfl_xor(a, 32, 64));
            const int t = f4w_scale_exp(a);
            const unsigned code = f4w_code8(v[2 * h], v[2 * h + 1], __uint_as_float((unsigned)(127 - t) << 23));
            if (h == 0) c.x = code; else c.y = code;
            sb |= (unsigned)(t + 127) << (8 * h);
        }
        dst[((size_t)rb * K64 + s) * 64 + lane] = c;
        if (lane < 16) scales[((size_t)rb * K64 + s) * 16 + lane] = (unsigned short)sb;
    }
}
}  // namespace

extern "C" {

size_t hpa_frag_fp4_bytes(int rows, int K) { return (size_t)((rows + 15) / 16) * 16 * (size_t)K / 2; }
size_t hpa_frag_mx_scale_bytes(int rows, int K) { return (size_t)((rows + 15) / 16) * 16 * (size_t)(K / 32); }

int hpa_pack_frag_fp4(const float* W, int N, int K, int ld, unsigned char* dst_codes, unsigned char* dst_scales) {
    HPA_REQUIRE(W && dst_codes && dst_scales && N > 0 && K > 0 && K % 64 == 0 && ld >= K && ld % 4 == 0 &&
                    ((size_t)W & 15) == 0 && ((size_t)dst_codes & 7) == 0 && ((size_t)dst_scales & 1) == 0,
                "pack_frag_fp4: bad shape (K % 64, ld % 4, 16-byte aligned W, 8-byte dst_codes, 2-byte dst_scales)");
    pack_frag_fp4_kernel<<<(unsigned)((N + 15) / 16), 256, 0, hpa_stream()>>>(
        W, N, K, ld, reinterpret_cast<uint2*>(dst_codes), reinterpret_cast<unsigned short*>(dst_scales));
    HPA_LAUNCH_CHECK();
    return 0;
}

// out4 = {variant, waves, row_blocks, col_tiles (variant 1) or rounds (variant
// 5)} of an fp4-weight GEMM left to the library (variant 0), after
// profiles/r20/w_fp4.txt.  The looped form in the fp8 table's shapes (waves by K
// alone) everywhere but the one shape where the A-resident form beat it by more
// than the larger of the two spreads: the XL fc (N = 6400, K = 1600) at M = 256,
// 37.0 against 40.5 us (spreads 1.1, 2.5), taken from M = 256 up (A re-reads
// grow with M; at M = 64 it loses 18.7 to 16.0).  4 waves, 2 row blocks, rounds
// auto, as measured.  Everywhere else the A-resident form lost or tied and is
// reached by variant = 5 only.
void hpa_fused_pick_fp4(int M, int N, int K, int* out4) {
    if (M >= 256 && N >= 6400 && K == 1600) {
        out4[0] = 5;
        out4[1] = 4;
        out4[2] = 2;
        out4[3] = 0;
        return;
    }
    const int small = (M + 15) / 16 < 8 && N <= 1024;
    out4[0] = 1;
    out4[1] = K >= 2048 ? 8 : 4;
    out4[2] = small ? 1 : 2;
    out4[3] = small ? 1 : 2;
}

}  // extern "C"
