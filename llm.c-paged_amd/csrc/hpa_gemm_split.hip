// hpa_gemm_split.hip -- the fused GEMMs on fp32 weights, multiplied on the bf16
// matrix pipe by exact operand splitting (hpa_gemm_fused variant 7).
//
// Contract, weight layout and epilogues are the looped fp32 kernel's
// (hpa_gemm_body.h gemm16_body): fp32 weights in the fp32 frag layout as they
// stand -- no repack, no second copy, nothing at init -- so an fp32 engine can
// switch between the two launch by launch.  What changes is the contraction:
// v_mfma_f32_16x16x4_f32 runs at one sixteenth of v_mfma_f32_16x16x32_bf16's
// rate, and an fp32 product costs six bf16 piece products here, which leaves
// 16 / 6 = 2.67x by instruction rates (an upper bound, not a measurement).
//
// Operands: lane l = (row l & 15, group g = l >> 4) of a 32-deep bf16 MFMA
// step s needs k = 32s + 4g + {0..3} and 32s + 16 + 4g + {0..3}: the two
// float4s the same lane loads from the fp32 frag layout at k16-steps 2s and
// 2s + 1 (hpa_gemm_bf16.hip's header), for A and for W alike.  A fragment is
// two 16-byte loads; nothing moves between lanes.
//
// Split (hpa_split3.h): each fragment is cut in registers into three bf16x8
// operands, x = hi + mid + lo exactly (piece 0 hi, 1 mid, 2 lo).  For pieces
// (a_i, w_j) the six products with i + j <= 2 are issued, each one MFMA into
// the same fp32 accumulator, smallest first:
//   (lo, hi) (hi, lo) (mid, mid) (mid, hi) (hi, mid) (hi, hi).
// Every bf16 x bf16 product is exact in fp32.  Left out: (mid, lo) (lo, mid)
// (lo, lo), below 2 * 2^-22 + 2^-30 < 2^-21 of |a||w| (|mid| < 2^-7 |x|,
// |lo| < 2^-15 |x|, truncation).
//
// Work split: the looped kernels', so the shared epilogue Epi<NW, EPI, MT, NTW>
// is used unchanged.  A workgroup owns MT 16-row blocks x NTW 16-column tiles;
// its NW waves divide the K range into contiguous runs of 32-deep steps, and
// Epi::finish folds them in wave order: a row's summation order depends on NW
// alone, never on MT, NTW or M.  Per step a wave loads and splits MT + NTW
// fragments -- each (row block, step) and (column tile, step) fragment is split
// by exactly one wave of a workgroup, and the MT x NTW reuse happens in
// registers, so the pieces are never staged in LDS -- and issues MT * NTW * 6
// MFMAs, term by term over all accumulators (consecutive MFMAs are independent
// when MT * NTW > 1).  Two steps are in flight: one being split and
// multiplied, the next one's 2 (MT + NTW) loads outstanding.
//
// LayerNorm: on load (ln4, fp32, K <= HPA_FUSED_LN_KMAX) before the split, or
// folded (ln_fold_c1): the row statistics are summed from the fp32 A fragments
// the wave holds (row_sums_add over k16-steps 2s, 2s + 1 in order) and applied
// in the epilogue.
//
// Registers: MT * NTW accumulators (4 each), 3 (MT + NTW) piece operands (4
// each) of the step being multiplied, 2 (MT + NTW) float4 of the step in
// flight.  At 4 x 4 that is 64 + 96 + 64; __launch_bounds__(NW * 64) gives a
// 4-wave workgroup 512 registers per lane and an 8-wave one 256, and (4, 4)
// exists at 4 waves only (its fold scratch passes the LDS at 8).
#include <math.h>

#include "hpa_gemm_body.h"
#include "hpa_split3.h"

namespace hpa_gemm {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
using hpa_split::u32x4;

// the three piece operands of the 8 k values (two float4s) of one lane
__device__ __forceinline__ void split_frag(float4 a, float4 b, u32x4* piece) {
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    hpa_split::split3x8(x, piece);
}

template <int NW, int EPI, int MT, int NTW>
__global__ __launch_bounds__(NW * 64) void gemm_split_kernel(FG p) {
    __shared__ __attribute__((aligned(16))) float smem[gemm16_lds_floats<NW, MT, NTW>()];
    constexpr int R = MT * 16;
    // the six piece products (A piece, W piece), smallest first
    constexpr int TA[6] = {2, 0, 1, 1, 0, 0};
    constexpr int TW[6] = {0, 2, 1, 0, 1, 0};
    float* lngb = smem;                         // LN weight [K], bias [K]; folded LN: the waves' row sums
    float* red = smem + 2 * HPA_FUSED_LN_KMAX;  // [NW][NTW][MT x 4][64]
    float* tile = red + NW * MT * NTW * 256;    // [NTW][R][17]
    float* lnst = tile + NTW * R * 17;          // [R][2]
    float* lnscr = lnst + 2 * R;                // [4R][2]

    int cx, ry;
    if (!xcd_tile(p, blockIdx.x, cx, ry)) return;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: the step bounds stay scalar
    const int nt0 = cx * NTW;
    const int row0 = ry * R;
    const int q4 = lane >> 4;

    // this wave's contiguous run of 32-deep steps
    const int K32 = p.K >> 5;
    const int per = (K32 + NW - 1) / NW;
    const int kb0 = w * per;
    const int nsteps = max(0, min(K32, kb0 + per) - kb0);
    const float4* __restrict__ wf[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j)  // tail tiles past ntn re-read the last tile (never stored)
        wf[j] = reinterpret_cast<const float4*>(p.w) + (size_t)min(nt0 + j, p.ntn - 1) * p.K16 * 64 + lane;
    const float4* __restrict__ xf = reinterpret_cast<const float4*>(p.x) + (size_t)ry * MT * p.K16 * 64 + lane;
    const size_t rbs = (size_t)p.K16 * 64;  // float4 stride between row blocks
    const bool fold = p.fold_c1 != nullptr;  // folded LN: raw A, statistics in the epilogue
    const bool ln_apply = p.ln_stats != nullptr && !fold;
    const float4* sg = reinterpret_cast<const float4*>(lngb) + q4;
    const float4* sb = reinterpret_cast<const float4*>(lngb + HPA_FUSED_LN_KMAX) + q4;

    struct Buf {
        float4 w[NTW][2], x[MT][2];
    };
    Buf A, Bb;
    // unconditional, clamped into [0, K32): a step past the wave's run re-reads
    // a valid fragment that comp never uses (a wave with no steps included)
    auto load = [&](Buf& f, int t) {
        const int k = min(kb0 + min(t, max(nsteps - 1, 0)), K32 - 1);
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            f.w[j][0] = wf[j][(size_t)(2 * k) * 64];
            f.w[j][1] = wf[j][(size_t)(2 * k + 1) * 64];
        }
#pragma unroll
        for (int r = 0; r < MT; ++r) {
            f.x[r][0] = xf[r * rbs + (size_t)(2 * k) * 64];
            f.x[r][1] = xf[r * rbs + (size_t)(2 * k + 1) * 64];
        }
    };
    load(A, 0);  // first operands in flight during the LN prologue

    float mu[MT], rs[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) mu[r] = rs[r] = 0.f;
    if (ln_apply) ln_prologue<NW, MT>(p, lngb, lnst, lnscr, row0, true, mu, rs);

    f32x4 acc[MT * NTW];
#pragma unroll
    for (int i = 0; i < MT * NTW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float fs1[MT], fs2[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) fs1[r] = fs2[r] = 0.f;

    auto comp = [&](Buf& f, int t) {
        if (t < nsteps) {
            const int k = kb0 + t;
            float4 g0, b0, g1, b1;
            if (ln_apply) {
                g0 = sg[4 * (2 * k)];
                b0 = sb[4 * (2 * k)];
                g1 = sg[4 * (2 * k + 1)];
                b1 = sb[4 * (2 * k + 1)];
            }
            u32x4 xa[MT][3], wb[NTW][3];
#pragma unroll
            for (int r = 0; r < MT; ++r) {
                float4 x0 = f.x[r][0], x1 = f.x[r][1];
                if (fold) {
                    row_sums_add(x0, fs1[r], fs2[r]);
                    row_sums_add(x1, fs1[r], fs2[r]);
                }
                if (ln_apply) {
                    x0 = ln4(x0, mu[r], rs[r], g0, b0);
                    x1 = ln4(x1, mu[r], rs[r], g1, b1);
                }
                split_frag(x0, x1, xa[r]);
            }
#pragma unroll
            for (int j = 0; j < NTW; ++j) split_frag(f.w[j][0], f.w[j][1], wb[j]);
#pragma unroll
            for (int term = 0; term < 6; ++term)
#pragma unroll
                for (int j = 0; j < NTW; ++j)
#pragma unroll
                    for (int r = 0; r < MT; ++r)
                        acc[j * MT + r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            __builtin_bit_cast(bf16x8, xa[r][TA[term]]), __builtin_bit_cast(bf16x8, wb[j][TW[term]]),
                            acc[j * MT + r], 0, 0, 0);
        }
    };
    // no exit between the two halves (gemm16_body's note): an odd step count
    // runs one empty half, comp skips steps >= nsteps
    for (int t = 0; t < nsteps; t += 2) {
        load(Bb, t + 1);
        comp(A, t);
        load(A, t + 2);
        comp(Bb, t + 1);
    }

    if (fold)  // [NW][R][2] over the LN weight area (unused when folded)
#pragma unroll
        for (int r = 0; r < MT; ++r) row_sums_publish(fs1[r], fs2[r], lngb + (w * R + 16 * r) * 2);
    Epi<NW, EPI, MT, NTW> epi;
    epi.prefetch(p, nt0, row0);
    epi.finish(p, acc, red, tile, nt0, row0, lngb);
}

template <int NW, int MT, int NTW>
static int launch_split_t(FG p, int epi) {
    const int gx = (p.ntn + NTW - 1) / NTW, gy = p.Mp / 16 / MT;
    p.gx = gx;
    p.gy = gy;
    dim3 grid((unsigned)(((gx + 7) / 8) * 8 * gy)), block(NW * 64);
    switch (epi) {
        case HPA_FEPI_QKV: gemm_split_kernel<NW, HPA_FEPI_QKV, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p); break;
        case HPA_FEPI_RESID: gemm_split_kernel<NW, HPA_FEPI_RESID, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p); break;
        case HPA_FEPI_GELU: gemm_split_kernel<NW, HPA_FEPI_GELU, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p); break;
        case HPA_FEPI_LOGITS: gemm_split_kernel<NW, HPA_FEPI_LOGITS, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p); break;
        case HPA_FEPI_SCORE: gemm_split_kernel<NW, HPA_FEPI_SCORE, MT, NTW><<<grid, block, 0, hpa_stream()>>>(p); break;
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused split: unknown epilogue");
    }
    HPA_LAUNCH_CHECK();
    return 0;
}

template <int NW>
static int launch_split_nw(const FG& p, int epi, int mt, int ntw) {
    switch (mt * 10 + ntw) {
        case 11: return launch_split_t<NW, 1, 1>(p, epi);
        case 12: return launch_split_t<NW, 1, 2>(p, epi);
        case 14: return launch_split_t<NW, 1, 4>(p, epi);
        case 21: return launch_split_t<NW, 2, 1>(p, epi);
        case 22: return launch_split_t<NW, 2, 2>(p, epi);
        case 24: return launch_split_t<NW, 2, 4>(p, epi);
        case 41: return launch_split_t<NW, 4, 1>(p, epi);
        case 42: return launch_split_t<NW, 4, 2>(p, epi);
        case 44:
            if constexpr (NW == 4) return launch_split_t<NW, 4, 4>(p, epi);
            return hpa_fail(__FILE__, __LINE__, "gemm_fused split: row_blocks 4 x col_tiles 4 needs waves 4 (LDS)");
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused split: row_blocks and col_tiles must be 1, 2 or 4");
    }
}

int launch_split(const FG& p, int epi, int nw, int mt, int ntw) {
    switch (nw) {
        case 4: return launch_split_nw<4>(p, epi, mt, ntw);
        case 8: return launch_split_nw<8>(p, epi, mt, ntw);
        default: return hpa_fail(__FILE__, __LINE__, "gemm_fused split: waves must be 4 or 8");
    }
}

}  // namespace hpa_gemm
