// hpa_gemm_fp8w.hip -- the fused decode GEMMs on fp8 (e4m3fn) weights:
// weight-only quantisation, one power-of-two scale per output channel
// (W8A16 beside an fp8 KV pool).  A sibling of gemm_b16_kernel
// (hpa_gemm_bf16.hip): same launches, epilogues and XCD-aware grid, the same
// MFMA (v_mfma_f32_16x16x32_bf16, fp32 accumulation) and the same A operand
// (LN'ed fp32 frag activations rounded to bf16 in registers), but the weights
// stream from HBM at ONE byte per element and are decoded to bf16 in
// registers, which is exact: every e4m3 value is a bf16 value.
//
// Numerics: code = e4m3fn_rne(clamp(w / s_n, -448, 448)) with s_n the smallest
// power of two with absmax_n / s_n <= 448 (exponent clamped to [-64, 64]; 1
// for an all-zero row).  The kernel sums a_k * decode(code_nk) in fp32 and
// multiplies the folded sum by s_n once, before the bias.  decode(code) * s_n
// is exactly a bf16 value, so the result is what the bf16-weight numerics
// give on the dequantised parameters W' = decode(code) * s.
//
// fp8 frag layout of a [rows][K] matrix (rows padded to 16, K % 64 == 0): the
// unit is (16-row block, 64-deep step s), 1 KiB contiguous, 16 bytes per lane.
// Lane l = (row l & 15, group g = l >> 4); its dword d (0..3) holds the codes
// of k = 64s + 16d + 4g + {0..3} -- the four k of the float4 the same lane
// loads from the fp32 frag layout at k16-step 4s + d.  Dwords (0, 1) are the B
// fragment of the first MFMA k-step of the unit, (2, 3) of the second, and
// the A fragments are pack_bf16 of the activations' float4 pairs (4s, 4s+1)
// and (4s+2, 4s+3): nothing is moved on either side, and one dwordx4 load
// feeds two MFMAs.
#include <math.h>

#include "hpa_gemm_body.h"

namespace hpa_gemm {

typedef __bf16 f8w_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 f8w_bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned f8w_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short f8w_u16x8 __attribute__((ext_vector_type(8)));

// four e4m3 codes (one dword) -> four bf16 in two dwords, exact.  gfx950 has
// the direct convert (v_cvt_scalef32_pk_bf16_fp8 at scale 1.0: one VALU
// instruction per two codes); the portable route is v_cvt_pk_f32_fp8 and the
// high halves of the two floats (v_perm_b32), two instructions per two codes.
__device__ __forceinline__ void e4m3x4_to_bf16(unsigned w, unsigned& lo, unsigned& hi) {
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8)
    lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
    hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
#else
    const hpa::e4m3_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const hpa::e4m3_f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    lo = __builtin_amdgcn_perm(__float_as_uint(a.y), __float_as_uint(a.x), 0x07060302u);
    hi = __builtin_amdgcn_perm(__float_as_uint(b.y), __float_as_uint(b.x), 0x07060302u);
#endif
}
// two dwords of codes (k = 16d + 4g + {0..3}, d = 0, 1 of an MFMA k-step) -> its B fragment
__device__ __forceinline__ f8w_bf16x8 f8w_frag(unsigned c0, unsigned c1) {
    f8w_u32x4 u;
    unsigned a, b;
    e4m3x4_to_bf16(c0, a, b);
    u[0] = a;
    u[1] = b;
    e4m3x4_to_bf16(c1, a, b);
    u[2] = a;
    u[3] = b;
    return __builtin_bit_cast(f8w_bf16x8, u);
}
__device__ __forceinline__ f8w_bf16x8 f8w_pack_a(float4 a, float4 b) {
    f8w_u16x8 u;
    u[0] = hpa::f32_to_bf16(a.x);
    u[1] = hpa::f32_to_bf16(a.y);
    u[2] = hpa::f32_to_bf16(a.z);
    u[3] = hpa::f32_to_bf16(a.w);
    u[4] = hpa::f32_to_bf16(b.x);
    u[5] = hpa::f32_to_bf16(b.y);
    u[6] = hpa::f32_to_bf16(b.z);
    u[7] = hpa::f32_to_bf16(b.w);
    return __builtin_bit_cast(f8w_bf16x8, u);
}

// 64-deep steps per trip, two trips in flight.  One step holds 4 * NTW dwords
// of weights and 16 * MT of activations per lane (the bf16 kernel's 32-deep
// step: 4 * NTW and 8 * MT): the activations, not the weights, size the trip
// here, so only the one-row-block shape carries two steps per trip (40
// registers a buffer against the bf16 kernel's 48)
template <int MT, int NTW>
constexpr int f8w_trip() {
    return (4 * MT + NTW) <= 5 ? 2 : 1;
}

// MT = 16-row blocks, NTW = 16-column tiles per workgroup, NW = waves sharing
// the K range in contiguous runs of 64-deep steps (wave w: steps [w * per,
// w * per + per) with per = ceil(K/64 / NW), folded in wave order; a wave past
// the end folds zeros): a row's summation order depends on NW only, never on
// MT, NTW or M.
template <int NW, int EPI, int MT, int NTW>
__global__ __launch_bounds__(NW * 64) void gemm_f8w_kernel(FG p, const float* __restrict__ w_scale) {
    constexpr int U = f8w_trip<MT, NTW>();
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
    const uint4* __restrict__ wf[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j)  // tail tiles past ntn re-read the last tile (never stored)
        wf[j] = reinterpret_cast<const uint4*>(p.w) + (size_t)min(nt0 + j, p.ntn - 1) * K64 * 64 + lane;
    const float4* __restrict__ xf = reinterpret_cast<const float4*>(p.x) + (size_t)ry * MT * p.K16 * 64 + lane;
    const size_t rbs = (size_t)p.K16 * 64;  // float4 stride between row blocks
    const bool ln_apply = p.ln_stats != nullptr;
    const float4* sg = reinterpret_cast<const float4*>(lngb) + q4;
    const float4* sb = reinterpret_cast<const float4*>(lngb + HPA_FUSED_LN_KMAX) + q4;

    struct Buf {
        uint4 w[U][NTW];
        float4 x[U][MT][4];
    };
    Buf A, Bb;
    auto load = [&](Buf& f, int t) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kb0 + min(t * U + u, nsteps - 1);  // clamped, unconditional (callers: nsteps > 0)
#pragma unroll
            for (int j = 0; j < NTW; ++j) f.w[u][j] = wf[j][(size_t)k * 64];
#pragma unroll
            for (int r = 0; r < MT; ++r)
#pragma unroll
                for (int d = 0; d < 4; ++d) f.x[u][r][d] = xf[r * rbs + (size_t)(4 * k + d) * 64];
        }
    };
    const int trips = (nsteps + U - 1) / U;
    if (trips > 0) load(A, 0);  // first operands in flight during the LN prologue

    // the scales of the columns this thread owns in the epilogue (its column
    // within a tile is fixed: NT is a multiple of 64), issued early as the
    // epilogue's own operands are
    float sc[E::EPT];
#pragma unroll
    for (int i = 0; i < E::EPT; ++i) {
        int j, lrow, lcol, row, col;
        E::where(threadIdx.x + i * E::NT, nt0, row0, j, lrow, lcol, row, col);
        sc[i] = (threadIdx.x + i * E::NT < NTW * E::TE && col < p.N) ? w_scale[col] : 1.f;
    }

    float mu[MT], rs[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) mu[r] = rs[r] = 0.f;
    if (ln_apply) ln_prologue<NW, MT>(p, lngb, lnst, lnscr, row0, true, mu, rs);

    f32x4 acc[MT * NTW];
#pragma unroll
    for (int i = 0; i < MT * NTW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto comp = [&](Buf& f, int t) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t * U + u < nsteps) {
                const int k = kb0 + t * U + u;
#pragma unroll
                for (int h = 0; h < 2; ++h) {  // the unit's two MFMA k-steps
                    f8w_bf16x8 xa[MT];
                    float4 g0, b0, g1, b1;
                    if (ln_apply) {
                        g0 = sg[4 * (4 * k + 2 * h)];
                        b0 = sb[4 * (4 * k + 2 * h)];
                        g1 = sg[4 * (4 * k + 2 * h + 1)];
                        b1 = sb[4 * (4 * k + 2 * h + 1)];
                    }
#pragma unroll
                    for (int r = 0; r < MT; ++r) {
                        float4 x0 = f.x[u][r][2 * h], x1 = f.x[u][r][2 * h + 1];
                        if (ln_apply) {
                            x0 = ln4(x0, mu[r], rs[r], g0, b0);
                            x1 = ln4(x1, mu[r], rs[r], g1, b1);
                        }
                        xa[r] = f8w_pack_a(x0, x1);
                    }
#pragma unroll
                    for (int j = 0; j < NTW; ++j) {  // decoded once, used by all MT row blocks
                        const f8w_bf16x8 wb = h == 0 ? f8w_frag(f.w[u][j].x, f.w[u][j].y) : f8w_frag(f.w[u][j].z, f.w[u][j].w);
#pragma unroll
                        for (int r = 0; r < MT; ++r)
                            acc[j * MT + r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[r], wb, acc[j * MT + r], 0, 0, 0);
                    }
                }
            }
        }
    };
    // unconditional loads and no exit between the halves, as gemm16_body: a
    // trip past the end re-reads the wave's last step and comp skips it
    for (int t = 0; t < trips; t += 2) {
        load(Bb, t + 1);
        comp(A, t);
        load(A, t + 2);
        comp(Bb, t + 1);
    }

    // the shared fold (wave order), each column's sum scaled once, then the shared epilogue
    E epi;
    epi.prefetch(p, nt0, row0);
    float vals[E::EPT];
    E::fold(acc, red, vals);
#pragma unroll
    for (int i = 0; i < E::EPT; ++i) vals[i] = __fmul_rn(vals[i], sc[i]);
    epi.apply(p, vals, tile, nt0, row0, nullptr);
}

template <int NW, int MT, int NTW>
static int launch_f8w_t(FG p, const float* w_scale, int epi) {
    const int gx = (p.ntn + NTW - 1) / NTW, gy = p.Mp / 16 / MT;
    p.gx = gx;
    p.gy = gy;
    dim3 grid((unsigned)(((gx + 7) / 8) * 8 * gy)), block(NW * 64);
    switch (epi) {
        case HPA_FEPI_QKV: gemm_f8w_kernel<NW, HPA_FEPI_QKV, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, w_scale); break;
        case HPA_FEPI_RESID: gemm_f8w_kernel<NW, HPA_FEPI_RESID, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, w_scale); break;
        case HPA_FEPI_GELU: gemm_f8w_kernel<NW, HPA_FEPI_GELU, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, w_scale); break;
        case HPA_FEPI_LOGITS: gemm_f8w_kernel<NW, HPA_FEPI_LOGITS, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, w_scale); break;
        case HPA_FEPI_SCORE: gemm_f8w_kernel<NW, HPA_FEPI_SCORE, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p, w_scale); break;
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused fp8 weights: unknown epilogue");
    }
    HPA_LAUNCH_CHECK();
    return 0;
}

template <int NW>
static int launch_f8w_nw(const FG& p, const float* w_scale, int epi, int mt, int ntw) {
    switch (mt * 10 + ntw) {
        case 11: return launch_f8w_t<NW, 1, 1>(p, w_scale, epi);
        case 21: return launch_f8w_t<NW, 2, 1>(p, w_scale, epi);
        case 41: return launch_f8w_t<NW, 4, 1>(p, w_scale, epi);
        case 22: return launch_f8w_t<NW, 2, 2>(p, w_scale, epi);
        case 42: return launch_f8w_t<NW, 4, 2>(p, w_scale, epi);
        default:
            return hpa_fail(__FILE__, __LINE__,
                            "gemm_fused fp8 weights: (row_blocks, col_tiles) in {(1,1), (2,1), (4,1), (2,2), (4,2)}");
    }
}

int launch_f8w(const FG& p, const float* w_scale, int epi, int nw, int mt, int ntw) {
    switch (nw) {
        case 4: return launch_f8w_nw<4>(p, w_scale, epi, mt, ntw);
        case 8: return launch_f8w_nw<8>(p, w_scale, epi, mt, ntw);
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused fp8 weights: waves must be 4 or 8");
    }
}

}  // namespace hpa_gemm

namespace {
// the power-of-two scale of a row from its absmax, exactly from the fp32
// fields: absmax = (1 + f) 2^e gives s = 2^(e - 8) when 1 + f <= 1.75 (448 =
// 1.75 x 2^8), else 2^(e - 7), so absmax / s lies in (224, 448].  The exponent
// is clamped to [-64, 64] (a zero, subnormal or < 224 x 2^-64 absmax: 2^-64
// and the row keeps what e4m3 resolves there; infinite or > 448 x 2^64: 2^64
// and the codes saturate at +-448).  An all-zero row: 1.
__device__ __forceinline__ int f8w_scale_exp(float absmax) {
    const unsigned u = __float_as_uint(absmax);
    const int ef = (int)((u >> 23) & 0xffu);
    const int t = ef == 0 ? -64 : ef - 127 - ((u & 0x7fffffu) <= 0x600000u ? 8 : 7);
    return absmax == 0.f ? 0 : max(-64, min(64, t));
}
__device__ __forceinline__ float f8w_pow2(int t) { return __uint_as_float((unsigned)(t + 127) << 23); }

// one 256-thread workgroup per 16-row block: 16 threads per row reduce its
// absmax (a maximum: the same in any order), then the block's units are
// written 16 bytes per thread in the layout above.  Padded rows: code 0, scale 1.
__global__ __launch_bounds__(256) void pack_frag_fp8_kernel(const float* __restrict__ src, int rows, int K, int ld,
                                                            uint4* __restrict__ dst, float* __restrict__ scale) {
    __shared__ float inv_s[16];
    const int rb = blockIdx.x;
    {
        const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
        const int m = rb * 16 + r;
        float a = 0.f;
        if (m < rows)
            for (int k = 4 * q; k < K; k += 64) {
                const float4 v = *reinterpret_cast<const float4*>(src + (size_t)m * ld + k);
                a = fmaxf(a, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
            }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
        if (q == 0) {
            const int t = f8w_scale_exp(a);
            inv_s[r] = f8w_pow2(-t);
            scale[m] = f8w_pow2(t);  // m < 16 * gridDim.x: the padded length
        }
    }
    __syncthreads();
    const int K64 = K >> 6;
    for (int i = threadIdx.x; i < K64 * 64; i += 256) {
        const int s = i >> 6, lane = i & 63;
        const int m = rb * 16 + (lane & 15);
        uint4 c = make_uint4(0u, 0u, 0u, 0u);
        if (m < rows) {
            const float inv = inv_s[lane & 15];
            const float* row = src + (size_t)m * ld + 64 * s + 4 * (lane >> 4);
            const float4 v0 = *reinterpret_cast<const float4*>(row);
            const float4 v1 = *reinterpret_cast<const float4*>(row + 16);
            const float4 v2 = *reinterpret_cast<const float4*>(row + 32);
            const float4 v3 = *reinterpret_cast<const float4*>(row + 48);
            c.x = hpa::f32x4_to_e4m3(v0.x, v0.y, v0.z, v0.w, inv);
            c.y = hpa::f32x4_to_e4m3(v1.x, v1.y, v1.z, v1.w, inv);
            c.z = hpa::f32x4_to_e4m3(v2.x, v2.y, v2.z, v2.w, inv);
            c.w = hpa::f32x4_to_e4m3(v3.x, v3.y, v3.z, v3.w, inv);
        }
        dst[((size_t)rb * K64 + s) * 64 + lane] = c;
    }
}
}  // namespace

extern "C" {

size_t hpa_frag_fp8_bytes(int rows, int K) { return (size_t)((rows + 15) / 16) * 16 * (size_t)K; }

int hpa_pack_frag_fp8(const float* W, int N, int K, int ld, unsigned char* dst_frag, float* scale) {
    HPA_REQUIRE(W && dst_frag && scale && N > 0 && K > 0 && K % 64 == 0 && ld >= K && ld % 4 == 0 &&
                    ((size_t)W & 15) == 0 && ((size_t)dst_frag & 15) == 0,
                "pack_frag_fp8: bad shape (K % 64, ld % 4, 16-byte aligned W and dst_frag)");
    pack_frag_fp8_kernel<<<(unsigned)((N + 15) / 16), 256, 0, hpa_stream()>>>(W, N, K, ld, reinterpret_cast<uint4*>(dst_frag),
                                                                            scale);
    HPA_LAUNCH_CHECK();
    return 0;
}

// waves by K alone (a row's summation order must not follow the batch): 8
// where every wave still gets >= 4 of the 64-deep steps (K >= 2048: fcproj),
// else 4 (K = 768: 3 steps a wave; 8 waves would leave two of them idle).
// Row blocks and column tiles as the bf16 table.
void hpa_fused_pick_fp8(int M, int N, int K, int* out3) {
    const int small = (M + 15) / 16 < 8 && N <= 1024;
    out3[0] = K >= 2048 ? 8 : 4;
    out3[1] = small ? 1 : 2;
    out3[2] = small ? 1 : 2;
}

}  // extern "C"
