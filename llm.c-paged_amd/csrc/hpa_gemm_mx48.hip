// hpa_gemm_mx48.hip -- the fused layer GEMMs as W4A8 on gfx950's block-scaled
// matrix instruction: MXFP4 weights (the codes and e8m0 bytes of
// hpa_gemm_fp4w.hip, in a second layout) against MXFP8 activations (e4m3 codes,
// one e8m0 scale per row and 32 consecutive k), multiplied undecoded by
// v_mfma_scale_f32_16x16x128_f8f6f4 (A = fp8: cbsz 0, B = fp4: blgp 4), which
// applies both scales to each lane's 32 consecutive k in hardware.  Three
// kernels: the weight pack (init time), the activation quantiser (once per
// GEMM, with the GEMM's LayerNorm) and the GEMM, whose waves load both
// operands as bytes and do no operand arithmetic.
//
// The instruction's operand map (16x16x128, found with one-hot operands on the
// device and pinned by the tests): lane l holds, of the fp4 B operand, column
// l & 15 and k = 32 (l >> 4) .. + 31 of the step, one nibble each, the lower k
// in the low nibble (4 registers); of the fp8 A operand (8 registers), row
// l & 15 and two runs of 16 k, one byte each: registers 0..3 k = 16 (l >> 4) ..
// + 15, registers 4..7 k = 64 + 16 (l >> 4) .. + 15.  Both scale operands are one
// e8m0 byte per lane, picked from the scale register by a byte select, and go
// by k alone: lane l's byte scales row / column l & 15 at k = 32 (l >> 4) .. + 31,
// whichever lanes hold those elements.
// C/D is the 16x16 map of every other MFMA here (column l & 15, rows 4 (l >>
// 4) + reg).  Every product decode(a) 2^ta decode(w) 2^tw is exact in fp32; the
// sums are fp32, inside the instruction over 128 k and in the accumulator.
//
// mx4 weight layout of W [N][K] (rows padded to 16, K % 32 == 0 padded to Kp =
// a multiple of 128 with code 0 / byte 127; S = Kp / 128 steps, S4 = ceil(S /
// 4)): codes [row block][S][64 lanes][16 B], lane l = row l & 15, group l >> 4;
// scales [row block][S4][64 lanes] dwords, byte i of dword d the lane's scale
// at step 4d + i.  A workspace of [M][K] activations: codes [row block][S][2
// halves][64 lanes][16 B] (half h of lane l = row l & 15, k = 64h + 16 (l >> 4)
// .. + 15: the A operand's registers 4h .. 4h + 3, one coalesced 16-byte load
// each), then the scales as the weights' (lane l: k = 32 (l >> 4) .. + 31).
#include <math.h>

#include <type_traits>

#include "hpa_gemm_body.h"
#include "hpa_mx_quant.h"

namespace hpa_gemm {

typedef int mx_i32x8 __attribute__((ext_vector_type(8)));

struct MX48 {             // the operands beside FG (p.w: the weight codes)
    const uint4* a;       // A codes
    const unsigned* as;   // A scale dwords
    const unsigned* ws;   // weight scale dwords
    int S, S4;            // 128-deep steps of the padded K, dwords of scales per lane
};

// ---- activation quantiser -------------------------------------------------
// t of a group from its absmax, from the fp32 fields: absmax = (1 + f) 2^E gives
// t = E - 8 when 1 + f <= 1.75 (448 = 1.75 x 2^8), else E - 7, so absmax / 2^t
// lies in (224, 448].  Clamped to [-64, 64]; an all-zero group: 0.
__device__ __forceinline__ int mx8_scale_exp(float absmax) {
    const unsigned u = __float_as_uint(absmax);
    const int ef = (int)((u >> 23) & 0xffu);
    const int t = ef == 0 ? -64 : ef - 127 - ((u & 0x7fffffu) <= 0x600000u ? 8 : 7);
    return absmax == 0.f ? 0 : max(-64, min(64, t));
}
// e4m3fn code of x = |v| 2^-t (exact: a power of two), round to nearest even,
// written out on the fp32 fields so every tie can be read here: from 2^-6 up
// the mantissa is cut to three bits (the carry runs into the exponent; x <=
// 448, so 0x7f is never reached), below it the code is x in units of 2^-9.
// The clamp acts only where t was clamped at 64.
__device__ __forceinline__ unsigned mx8_code(float v, float inv) {
    const float x = fminf(fabsf(v) * inv, 448.f);
    const unsigned u = __float_as_uint(x);
    const unsigned c = x >= 0.015625f ? ((u + 0x7ffffu + ((u >> 20) & 1u)) >> 20) - 960u : (unsigned)rintf(x * 512.f);
    return c | ((__float_as_uint(v) >> 24) & 0x80u);
}
__device__ __forceinline__ unsigned mx8_code4(float4 x, float inv) {
    return mx8_code(x.x, inv) | mx8_code(x.y, inv) << 8 | mx8_code(x.z, inv) << 16 | mx8_code(x.w, inv) << 24;
}
__device__ __forceinline__ float absmax4(float4 a) {
    return fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w)));
}

// One 256-thread workgroup per (16-row block, four steps); wave w takes step s
// = 4 sq + w in ONE pass over A: lane (row r, quarter q) of the fp32 frag
// layout loads its eight float4 of the step (k16-steps 8s .. 8s + 7; the MX
// group g is the pair 2g, 2g + 1, spread over the row's four lanes), applies
// the LayerNorm, takes each group's absmax across the four lanes by two
// shuffles (a maximum: the same in any order), and stores its dword of codes
// per k16-step i straight into the operand order: half i >> 2, lane r + 16 (i
// & 3), dword q -- 256 contiguous bytes per k16-step and wave.  Lane q == g
// writes the group's scale byte, at lane r + 16g.  Rows >= M, k >= K and the
// steps that fill the last scale dword: code 0, byte 127.  Every workgroup
// stages all of ln_w / ln_b through the shared ln_prologue; measured, the
// kernel's time is launch latency and does not move with K or LN.
__global__ __launch_bounds__(256) void quant_mxfp8_kernel(FG p, unsigned* __restrict__ codes,
                                                          unsigned char* __restrict__ scales, int S, int S4) {
    __shared__ __attribute__((aligned(16))) float smem[2 * HPA_FUSED_LN_KMAX + 10 * 16];
    float* lngb = smem;
    float* lnst = smem + 2 * HPA_FUSED_LN_KMAX;
    float* lnscr = lnst + 32;
    const int rb = blockIdx.x / S4, sq = blockIdx.x - rb * S4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int s = 4 * sq + w;
    const bool ln_apply = p.ln_stats != nullptr;
    const bool live = s < S && rb * 16 + r < p.M;

    float4 x[8];
    const float4* xf = reinterpret_cast<const float4*>(p.x) + (size_t)rb * p.K16 * 64 + lane;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        x[i] = live && 8 * s + i < p.K16 ? xf[(size_t)(8 * s + i) * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
    float mu[1] = {0.f}, rs[1] = {0.f};
    if (ln_apply) ln_prologue<4, 1>(p, lngb, lnst, lnscr, rb * 16, true, mu, rs);
    unsigned char* sb = scales + ((size_t)(rb * S4 + sq) * 64) * 4 + w;
    if (s >= S) {
        sb[4 * lane] = 127;
        return;
    }
    const float4* sg = reinterpret_cast<const float4*>(lngb) + q;
    const float4* sbv = reinterpret_cast<const float4*>(lngb + HPA_FUSED_LN_KMAX) + q;
    unsigned* dst = codes + ((size_t)(rb * S + s) * 128) * 4 + q;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float4 a = x[2 * g], b = x[2 * g + 1];
        if (ln_apply && live && 8 * s + 2 * g < p.K16) {  // K % 32 == 0: a group is whole
            a = ln4(a, mu[0], rs[0], sg[4 * (8 * s + 2 * g)], sbv[4 * (8 * s + 2 * g)]);
            b = ln4(b, mu[0], rs[0], sg[4 * (8 * s + 2 * g + 1)], sbv[4 * (8 * s + 2 * g + 1)]);
        }
        float m = fmaxf(absmax4(a), absmax4(b));
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        const int t = mx8_scale_exp(m);
        const float inv = __uint_as_float((unsigned)(127 - t) << 23);
        dst[(size_t)(64 * (g >> 1) + r + 16 * ((2 * g) & 3)) * 4] = mx8_code4(a, inv);
        dst[(size_t)(64 * (g >> 1) + r + 16 * ((2 * g + 1) & 3)) * 4] = mx8_code4(b, inv);
        if (q == g) sb[4 * (r + 16 * g)] = (unsigned char)(t + 127);
    }
}

static int quant_mxfp8(const FG& p, void* ws) {
    const int S = (p.K + 127) / 128, S4 = (S + 3) / 4, nrb = p.Mp / 16;
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    quant_mxfp8_kernel<<<(unsigned)(nrb * S4), 256, 0, hpa_stream()>>>(p, reinterpret_cast<unsigned*>(base),
                                                                       base + (size_t)p.Mp * S * 128, S, S4);
    HPA_LAUNCH_CHECK();
    return 0;
}

// ---- the GEMM ---------------------------------------------------------------
// steps per trip (two trips in flight): a step is 4 NTW weight and 8 MT
// activation registers
template <int MT, int NTW>
constexpr int mx48_trip() {
    return MT == 1 ? 4 : 2;
}
template <int NW, int MT, int NTW>
constexpr int mx48_lds_floats() {
    return NW * MT * NTW * 256 + NTW * MT * 16 * 17;
}

// MT = 16-row blocks, NTW = 16-column tiles per workgroup, NW = waves sharing K
// in contiguous runs of 128-deep steps (wave w: steps [w * per, w * per + per),
// per = ceil(S / NW), folded in wave order; a wave past the end folds zeros): a
// row's summation order depends on NW only.  Both operands stream straight
// into registers a trip ahead, the weights with one 16-byte load per lane and
// step, the activations with two.  The scale dwords hold four steps; a trip
// starts at any step, so it loads the dword of its first step and the next one
// and v_alignbyte brings the trip's bytes to byte 0 up: step u of the trip is
// then the instruction's byte select u, a constant.
template <int NW, int EPI, int MT, int NTW>
__global__ __launch_bounds__(NW * 64) void gemm_mx48_kernel(FG p, MX48 q) {
    constexpr int U = mx48_trip<MT, NTW>();
    using E = Epi<NW, EPI, MT, NTW>;
    __shared__ __attribute__((aligned(16))) float smem[mx48_lds_floats<NW, MT, NTW>()];
    float* red = smem;                        // [NW][NTW][MT x 4][64]
    float* tile = red + NW * MT * NTW * 256;  // [NTW][R][17]

    int cx, ry;
    if (!xcd_tile(p, blockIdx.x, cx, ry)) return;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: scalar step bounds
    const int nt0 = cx * NTW;
    const int row0 = ry * MT * 16;
    const int S = q.S, S4 = q.S4;
    const int per = (S + NW - 1) / NW;
    const int kb0 = w * per;
    const int nsteps = max(0, min(S, kb0 + per) - kb0);

    const uint4* __restrict__ wf[NTW];
    const unsigned* __restrict__ wsf[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {  // tail tiles past ntn re-read the last tile (never stored)
        const size_t t = (size_t)min(nt0 + j, p.ntn - 1);
        wf[j] = reinterpret_cast<const uint4*>(p.w) + t * S * 64 + lane;
        wsf[j] = q.ws + t * S4 * 64 + lane;
    }
    const uint4* __restrict__ af = q.a + (size_t)ry * MT * S * 128 + lane;
    const unsigned* __restrict__ asf = q.as + (size_t)ry * MT * S4 * 64 + lane;
    const size_t arb = (size_t)S * 128, asrb = (size_t)S4 * 64;  // strides between row blocks

    struct Buf {
        uint4 w[U][NTW], a[U][MT][2];
        unsigned ws[2][NTW], as[2][MT];
    };
    Buf A, B;
    // clamped, unconditional loads (callers: nsteps > 0): a step past the
    // wave's end re-reads its last step and comp skips it
    auto load = [&](Buf& f, int t) {
        const int k0 = kb0 + min(t * U, nsteps - 1);
        const int d0 = k0 >> 2, d1 = min(d0 + 1, S4 - 1);
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            f.ws[0][j] = wsf[j][(size_t)d0 * 64];
            f.ws[1][j] = wsf[j][(size_t)d1 * 64];
        }
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            f.as[0][r] = asf[r * asrb + (size_t)d0 * 64];
            f.as[1][r] = asf[r * asrb + (size_t)d1 * 64];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kb0 + min(t * U + u, nsteps - 1);
#pragma unroll
            for (int j = 0; j < NTW; ++j) f.w[u][j] = wf[j][(size_t)k * 64];
#pragma unroll
            for (int r = 0; r < MT; ++r) {
                f.a[u][r][0] = af[r * arb + (size_t)k * 128];
                f.a[u][r][1] = af[r * arb + (size_t)k * 128 + 64];
            }
        }
    };
    const int trips = (nsteps + U - 1) / U;
    if (trips > 0) load(A, 0);

    f32x4 acc[MT * NTW];
#pragma unroll
    for (int i = 0; i < MT * NTW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto comp = [&](Buf& f, int t) {
        const unsigned sh = (unsigned)(kb0 + t * U) & 3u;
        unsigned wsc[NTW], asc[MT];
#pragma unroll
        for (int j = 0; j < NTW; ++j) wsc[j] = __builtin_amdgcn_alignbyte(f.ws[1][j], f.ws[0][j], sh);
#pragma unroll
        for (int r = 0; r < MT; ++r) asc[r] = __builtin_amdgcn_alignbyte(f.as[1][r], f.as[0][r], sh);
        auto step = [&](auto uc) {
            constexpr int u = decltype(uc)::value;
            if constexpr (u < U) if (t * U + u < nsteps) {
                constexpr int uu = u;
#pragma unroll
                for (int j = 0; j < NTW; ++j) {
                    const uint4 c = f.w[uu][j];
                    const mx_i32x8 wb = {(int)c.x, (int)c.y, (int)c.z, (int)c.w, 0, 0, 0, 0};
#pragma unroll
                    for (int r = 0; r < MT; ++r) {
                        const uint4 a0 = f.a[uu][r][0], a1 = f.a[uu][r][1];
                        const mx_i32x8 xa = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w,
                                             (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
                        acc[j * MT + r] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                            xa, wb, acc[j * MT + r], 0, 4, u, (int)asc[r], u, (int)wsc[j]);
                    }
                }
            }
        };
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{});
        step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 3>{});
    };
    // no exit between the halves, as gemm16_body
    for (int t = 0; t < trips; t += 2) {
        load(B, t + 1);
        comp(A, t);
        load(A, t + 2);
        comp(B, t + 1);
    }

    // the shared fold (wave order), then the shared epilogue
    E epi;
    epi.prefetch(p, nt0, row0);
    float vals[E::EPT];
    E::fold(acc, red, vals);
    epi.apply(p, vals, tile, nt0, row0, nullptr);
}

template <int NW, int MT, int NTW>
static int launch_mx48_t(FG p, const MX48& q, int epi) {
    const int gx = (p.ntn + NTW - 1) / NTW, gy = p.Mp / 16 / MT;
    p.gx = gx;
    p.gy = gy;
    dim3 grid((unsigned)(((gx + 7) / 8) * 8 * gy)), block(NW * 64);
    switch (epi) {
        case HPA_FEPI_QKV: gemm_mx48_kernel<NW, HPA_FEPI_QKV, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, q); break;
        case HPA_FEPI_RESID: gemm_mx48_kernel<NW, HPA_FEPI_RESID, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, q); break;
        default: gemm_mx48_kernel<NW, HPA_FEPI_GELU, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, q); break;
    }
    HPA_LAUNCH_CHECK();
    return 0;
}

template <int NW>
static int launch_mx48_nw(const FG& p, const MX48& q, int epi, int mt, int ntw) {
    switch (mt * 10 + ntw) {
        case 11: return launch_mx48_t<NW, 1, 1>(p, q, epi);
        case 21: return launch_mx48_t<NW, 2, 1>(p, q, epi);
        case 41: return launch_mx48_t<NW, 4, 1>(p, q, epi);
        case 22: return launch_mx48_t<NW, 2, 2>(p, q, epi);
        default: return launch_mx48_t<NW, 4, 2>(p, q, epi);
    }
}

// the quantiser, then the GEMM, on the current stream; every refusal comes
// before the first launch
int launch_mx48(const FG& p, const unsigned char* gscale, void* a_ws, int epi, int nw, int mt, int ntw) {
    HPA_REQUIRE(epi == HPA_FEPI_QKV || epi == HPA_FEPI_RESID || epi == HPA_FEPI_GELU,
                "gemm_fused W4A8: epilogue QKV, RESID or GELU");
    HPA_REQUIRE(nw == 4 || nw == 8, "gemm_fused W4A8: waves must be 4 or 8");
    const int shape = mt * 10 + ntw;
    HPA_REQUIRE(shape == 11 || shape == 21 || shape == 41 || shape == 22 || shape == 42,
                "gemm_fused W4A8: (row_blocks, col_tiles) in {(1,1), (2,1), (4,1), (2,2), (4,2)}");
    HPA_REQUIRE(((size_t)p.w & 15) == 0 && ((size_t)gscale & 3) == 0 && ((size_t)a_ws & 15) == 0,
                "gemm_fused W4A8: 16-byte aligned codes and workspace, 4-byte aligned scales");
    MX48 q;
    q.S = (p.K + 127) / 128;
    q.S4 = (q.S + 3) / 4;
    q.a = reinterpret_cast<const uint4*>(a_ws);
    q.as = reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(a_ws) + (size_t)p.Mp * q.S * 128);
    q.ws = reinterpret_cast<const unsigned*>(gscale);
    if (quant_mxfp8(p, a_ws)) return 1;
    return nw == 4 ? launch_mx48_nw<4>(p, q, epi, mt, ntw) : launch_mx48_nw<8>(p, q, epi, mt, ntw);
}

}  // namespace hpa_gemm

namespace {
__device__ __forceinline__ unsigned mx4_code8(float4 a, float4 b, float inv) {
    return f4w_code(a.x, inv) | f4w_code(a.y, inv) << 4 | f4w_code(a.z, inv) << 8 | f4w_code(a.w, inv) << 12 |
           f4w_code(b.x, inv) << 16 | f4w_code(b.y, inv) << 20 | f4w_code(b.z, inv) << 24 | f4w_code(b.w, inv) << 28;
}

// one 256-thread workgroup per 16-row block; each wave takes steps s = wave,
// wave + 4, ... < 4 S4: lane (row, g) reads its group's 32 consecutive floats of
// the row, so the absmax needs no other lane, and writes its 16 bytes of codes
// and its scale byte.  Padded rows, k >= K and the steps that fill the last
// scale dword: code 0, byte 127.
__global__ __launch_bounds__(256) void pack_frag_mx4_kernel(const float* __restrict__ src, int rows, int K, int ld,
                                                            uint4* __restrict__ dst, unsigned char* __restrict__ scales,
                                                            int S, int S4) {
    const int rb = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int m = rb * 16 + (lane & 15);
    for (int s = threadIdx.x >> 6; s < 4 * S4; s += 4) {
        unsigned char* sb = scales + ((size_t)(rb * S4 + (s >> 2)) * 64 + lane) * 4 + (s & 3);
        if (s >= S) {
            *sb = 127;
            continue;
        }
        const int k0 = 128 * s + 32 * (lane >> 4);
        float4 v[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) v[d] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < rows && k0 < K) {
            const float* row = src + (size_t)m * ld + k0;
#pragma unroll
            for (int d = 0; d < 8; ++d) v[d] = *reinterpret_cast<const float4*>(row + 4 * d);
        }
        float a = 0.f;
#pragma unroll
        for (int d = 0; d < 8; ++d) a = fmaxf(a, hpa_gemm::absmax4(v[d]));
        const int t = f4w_scale_exp(a);
        const float inv = __uint_as_float((unsigned)(127 - t) << 23);
        dst[((size_t)rb * S + s) * 64 + lane] =
            make_uint4(mx4_code8(v[0], v[1], inv), mx4_code8(v[2], v[3], inv), mx4_code8(v[4], v[5], inv),
                       mx4_code8(v[6], v[7], inv));
        *sb = (unsigned char)(t + 127);
    }
}
}  // namespace

extern "C" {

size_t hpa_frag_mx4_bytes(int rows, int K) { return (size_t)((rows + 15) / 16) * 16 * (size_t)((K + 127) / 128) * 64; }
size_t hpa_frag_mx4_scale_bytes(int rows, int K) {
    return (size_t)((rows + 15) / 16) * (size_t)(((K + 127) / 128 + 3) / 4) * 256;
}
size_t hpa_mxfp8_workspace_bytes(int M, int K) {
    return (size_t)((M + 15) / 16) * 16 * (size_t)((K + 127) / 128) * 128 + hpa_frag_mx4_scale_bytes(M, K);
}

int hpa_pack_frag_mx4(const float* W, int N, int K, int ld, unsigned char* dst_codes, unsigned char* dst_scales) {
    HPA_REQUIRE(W && dst_codes && dst_scales && N > 0 && K > 0 && K % 32 == 0 && ld >= K && ld % 4 == 0 &&
                    ((size_t)W & 15) == 0 && ((size_t)dst_codes & 15) == 0 && ((size_t)dst_scales & 3) == 0,
                "pack_frag_mx4: bad shape (K % 32, ld % 4, 16-byte aligned W and dst_codes, 4-byte dst_scales)");
    const int S = (K + 127) / 128;
    pack_frag_mx4_kernel<<<(unsigned)((N + 15) / 16), 256, 0, hpa_stream()>>>(
        W, N, K, ld, reinterpret_cast<uint4*>(dst_codes), dst_scales, S, (S + 3) / 4);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_quant_mxfp8_rows(const float* x_frag, int M, int K, const float* ln_stats, int ln_ntiles, const float* ln_w,
                         const float* ln_b, void* ws) {
    HPA_REQUIRE(x_frag && ws && M > 0 && K > 0 && K % 32 == 0 && ((size_t)ws & 15) == 0,
                "quant_mxfp8_rows: bad shape (K % 32, 16-byte aligned workspace)");
    HPA_REQUIRE(!ln_stats || (ln_w && ln_b && ln_ntiles > 0 && K <= hpa_gemm::HPA_FUSED_LN_KMAX),
                "quant_mxfp8_rows: LN params (K <= 2048)");
    hpa_gemm::FG p = {};
    p.x = x_frag;
    p.M = M;
    p.Mp = (M + 15) / 16 * 16;
    p.K = K;
    p.K16 = K / 16;
    p.ln_stats = ln_stats;
    p.ln_ntiles = ln_ntiles;
    p.ln_w = ln_w;
    p.ln_b = ln_b;
    return hpa_gemm::quant_mxfp8(p, ws);
}

// out4 = {variant (1), waves, row_blocks, col_tiles} of a W4A8 GEMM left to the
// library (variant 0), after profiles/r21/w_mx48.txt (s).  4 waves everywhere: 8
// never won by more than the spread, at any K (a 128-deep step leaves 6 .. 50
// steps to share), and lost up to 2x at M = 1024.  (1, 1) for the narrow GEMMs
// below 8 row blocks, as the fp4 table; (4, 2) for the deep, tall ones (XL
// fcproj at M = 1024: 49.7 against 62.7 us); (2, 2) elsewhere, within the
// spread of the best shape at every measured point.
void hpa_fused_pick_mx48(int M, int N, int K, int* out4) {
    const int small = (M + 15) / 16 < 8 && N <= 1024;
    const int deep = K >= 4096 && M >= 512;
    out4[0] = 1;
    out4[1] = 4;
    out4[2] = small ? 1 : deep ? 4 : 2;
    out4[3] = small ? 1 : 2;
}

}  // extern "C"
