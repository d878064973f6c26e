// hpa_chain8.hip -- chain form 8 of hpa_decode_layer (gfx950): the chain for
// wide layers.
// GPT-2 XL (C = 1600, NH = 25): the same persistent
// chain attproj -> fc -> fcproj -> qkv(l+1) as form 6, sized for GEMMs that
// are MFMA-bound (3.9 GFLOP per layer at B = 64, 25 us at the fp32 rate):
//   * one unit of all 12 waves per workgroup = (row block, up to XT_MAX
//     16-column tiles[, fcproj K part]), T per phase chosen on the host so
//     the units fill the CUs (B = 64: attproj 2, fc 7, fcproj 7, qkv 5 tiles);
//     tile groups are padded to a multiple of 8 so the row blocks of a weight
//     tile land on one XCD and re-read it from that L2;
//   * a wave holds its K range of the A rows (K16 / 12 steps, 8 or 9 at XL)
//     once per phase and streams its weight fragments tile by tile, double
//     buffered: the phase's first tile is loaded before its wait;
//   * every tile's accumulators stay in registers until one LDS fold of all
//     T tiles; epilogues are 16-byte as in form 6;
//   * waits per row block; fcproj's 4 K parts (of C each) are combined by the
//     last part to draw its ticket, in part order.
// A wave's K range depends only on K, so a row's sums never depend on B.
#include "hpa_layer_common.h"

#ifndef HPA_CX_SB
#define HPA_CX_SB 1  // A/B builds: 0 = no scheduling barrier after form 8's A loads
#endif
namespace {
#ifdef HPA_LAYER_TRACE
__device__ unsigned long long g_pl_trace[64][256][16];
// the fc phase of one layer, per wave (s_memtime, shader clock): [0] A
// loads issued, [1 + q] half-tile q's MFMAs issued, [15] loop done
__device__ unsigned long long g_cx_wave[256][12][16];
#endif

namespace cx {
using namespace chain;  // NW, the counters X1 / H / X2 / kCtr, wait6, arrive6, publish6, fold_t, ln_fold4
constexpr int XT_MAX = 7;

template <int MAXS>
__device__ __forceinline__ void ld_tile(const float* W, int K16W, int j, int kb, int s0, int ns, bool nt,
                                        float4 (&wr)[MAXS]) {
    const float4* wf = reinterpret_cast<const float4*>(W) + ((size_t)j * K16W + kb + s0) * 64 + (threadIdx.x & 63);
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < ns) wr[s] = nt ? ld_nt(wf + (size_t)s * 64) : wf[(size_t)s * 64];
}

template <int MAXS>
__device__ __forceinline__ f32x4 chain_tile(const float4 (&xv)[MAXS], const float4 (&wr)[MAXS], int ns) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < ns) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].x, wr[s].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].y, wr[s].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].z, wr[s].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].w, wr[s].w, acc, 0, 0, 0);
        }
    return acc;
}

struct SmemX {
    float red[NW * XT_MAX * 256];
    float wsum[NW * 32];
    float tile[XT_MAX * 16 * 17];
    int s_ok;
    int s_last;
};

// the unit body up to the LDS fold: A (its K range of row block rb, sc1),
// row sums (STATS), then the nt tiles j0.. streamed in half-tiles (HS k16
// steps of the wave's range) through four register sets rotating by name,
// three half-tiles ahead (wr01 holds tile 0, loaded before the caller's
// wait); accumulators -> red[w][t].  One whole tile ahead left the XL fc
// phase at 19 us for 11.7 us of MFMA issue (profiles/r4/traces): a tile's
// 100 KB per CU did not land within one tile's MFMAs; two whole tiles ahead
// need 168 VGPRs + spills.
template <int MAXS>
struct HalfT {
    static constexpr int HS = (MAXS + 1) / 2;
};

template <int MAXS>
__device__ __forceinline__ void ld_half(const float* W, int K16W, int j, int kb, int s0, int ns, int h, bool nt,
                                        float4 (&wr)[HalfT<MAXS>::HS]) {
    constexpr int HS = HalfT<MAXS>::HS;
    const float4* wf = reinterpret_cast<const float4*>(W) + ((size_t)j * K16W + kb + s0 + h * HS) * 64 + (threadIdx.x & 63);
#pragma unroll
    for (int s = 0; s < HS; ++s)
        if (h * HS + s < ns) wr[s] = nt ? ld_nt(wf + (size_t)s * 64) : wf[(size_t)s * 64];
}

template <int MAXS>
__device__ __forceinline__ void chain_half(const float4 (&xv)[MAXS], const float4 (&wr)[HalfT<MAXS>::HS], int ns, int h,
                                           f32x4& acc) {
    constexpr int HS = HalfT<MAXS>::HS;
#pragma unroll
    for (int s = 0; s < HS; ++s)
        if (h * HS + s < ns) {
            const float4 x = xv[h * HS + s];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, wr[s].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, wr[s].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, wr[s].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, wr[s].w, acc, 0, 0, 0);
        }
}

template <int MAXS>
struct Tile0 {  // tile 0's two halves, loaded before the caller's wait
    float4 h0[HalfT<MAXS>::HS], h1[HalfT<MAXS>::HS];
};

template <int MAXS>
__device__ __forceinline__ void ld_tile0(const float* W, int K16W, int j, int kb, int s0, int ns, bool nt, Tile0<MAXS>& t0) {
    ld_half<MAXS>(W, K16W, j, kb, s0, ns, 0, nt, t0.h0);
    ld_half<MAXS>(W, K16W, j, kb, s0, ns, 1, nt, t0.h1);
}

template <int MAXS, bool STATS>
__device__ __forceinline__ void unit_body(const float* A, int K16A, const float* W, int K16W, int rb, int kb, int j0,
                                          int ntl, int s0, int ns, bool nt, Tile0<MAXS>& t0, float* red,
                                          float& fs1, float& fs2, bool wtrace = false) {
    (void)wtrace;
    constexpr int HS = HalfT<MAXS>::HS;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float4 xv[MAXS];
    const int off = ((rb * K16A + kb + s0) * 64 + lane) * 16;
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < ns) xv[s] = hpa::load_wt16(A, off + s * 1024);
#if HPA_CX_SB
    __builtin_amdgcn_sched_barrier(0);  // every A load in flight before the first MFMA (see mfma_t)
#endif
    CX_WSTAMP(wtrace, 0);
    if (STATS)
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) hpa_gemm::row_sums_add(xv[s], fs1, fs2);
    // half-tile q = 2t + h in set q % 4: sets 0, 1 = tile 0 (t0), 2, 3 here
    float4 w2[HS], w3[HS];
    if (ntl > 1) {
        ld_half<MAXS>(W, K16W, j0 + 1, kb, s0, ns, 0, nt, w2);
        ld_half<MAXS>(W, K16W, j0 + 1, kb, s0, ns, 1, nt, w3);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 2 * XT_MAX; ++q) {
        const int t = q >> 1, h = q & 1;
        if (t >= ntl) break;
        // half-tile q + 3 into the set half-tile q - 1 used (q % 4 == 0: set 3 is tile 1's half 1, still live)
        const int qn = q + 3;
        if (q >= 1 && (qn >> 1) < ntl) {
            if (qn % 4 == 0)
                ld_half<MAXS>(W, K16W, j0 + (qn >> 1), kb, s0, ns, qn & 1, nt, t0.h0);
            else if (qn % 4 == 1)
                ld_half<MAXS>(W, K16W, j0 + (qn >> 1), kb, s0, ns, qn & 1, nt, t0.h1);
            else if (qn % 4 == 2)
                ld_half<MAXS>(W, K16W, j0 + (qn >> 1), kb, s0, ns, qn & 1, nt, w2);
            else
                ld_half<MAXS>(W, K16W, j0 + (qn >> 1), kb, s0, ns, qn & 1, nt, w3);
        }
        if (q % 4 == 0)
            chain_half<MAXS>(xv, t0.h0, ns, h, acc);
        else if (q % 4 == 1)
            chain_half<MAXS>(xv, t0.h1, ns, h, acc);
        else if (q % 4 == 2)
            chain_half<MAXS>(xv, w2, ns, h, acc);
        else
            chain_half<MAXS>(xv, w3, ns, h, acc);
        CX_WSTAMP(wtrace, 1 + q);
        if (h == 1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) red[(w * XT_MAX + t) * 256 + g * 64 + lane] = acc[g];
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    CX_WSTAMP(wtrace, 15);
}

}  // namespace cx

template <int NH, int P, bool BF>
__global__ __launch_bounds__(768) void decode_chainx_kernel(KA args) {
    using namespace cx;
    constexpr int C = 64 * NH, K16 = C / 16, NCT = C / 16;
    constexpr int MAXS = (K16 + NW - 1) / NW;
    const KA& a = *(const KA*)(const void*)__builtin_amdgcn_kernarg_segment_ptr();
    (void)args;
    __shared__ SmemX sm;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = threadIdx.x;
    const int bid = blockIdx.x;
    const int R = a.R;
    const bool nt = R == 1;
    const int s0 = w * K16 / NW, ns = (w + 1) * K16 / NW - s0;  // this wave's k16 steps of a K = C range
    const int et = tid >> 6, er = (tid & 63) >> 2, eq = tid & 3;
    int* tick = a.ctr + kCtr;
    PL_STAMP(t_start);
    PL_STORE(0, t_start);
    float fs1 = 0.f, fs2 = 0.f;
    cx::Tile0<MAXS> t0w;
    // B: attproj(l): res2 = res + att . Wap^T + b
    {
        const int T = a.xt[0], NG = a.xng[0];
        const int g = bid % NG, rb = bid / NG, j0 = g * T;
        const bool has = rb < R && j0 < NCT;
        const int ntl = has ? min(T, NCT - j0) : 0;
        if (has) cx::ld_tile0<MAXS>(a.w_ap, K16, j0, 0, s0, ns, nt, t0w);
        const bool ep = tid < ntl * 64;
        const int row = rb * 16 + er, col = (j0 + et) * 16 + 4 * eq;
        const int fi = ep ? (int)(hpa::frag_index(row, col, C) * 4) : 0;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f), rv = bv;
        if (ep) {
            bv = ld4(a.b_ap + col);
            rv = hpa::load_wt16(a.res, fi);
        }
        if (has) unit_body<MAXS, false>(a.att, K16, a.w_ap, K16, rb, 0, j0, ntl, s0, ns, nt, t0w, sm.red, fs1, fs2);
        lds_barrier();
        if (ep) {
            float4 v = fold_t<XT_MAX>(sm.red, et, er, eq);
            v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            v = row < a.B ? make_float4(rv.x + v.x, rv.y + v.y, rv.z + v.z, rv.w + v.w) : make_float4(0.f, 0.f, 0.f, 0.f);
            hpa::store_wt16(a.res2, fi, v);
        }
        publish6(a, X1 + rb, has);
    }
    PL_MARK(5);
    // C: fc(l): fch = gelu(LN2(res2) . Wfc^T + b), LN folded
    {
        constexpr int NJ = 4 * NCT;
        const int T = a.xt[1], NG = a.xng[1];
        const int g = bid % NG, rb = bid / NG, j0 = g * T;
        const bool has = rb < R && j0 < NJ;
        const int ntl = has ? min(T, NJ - j0) : 0;
        if (has) cx::ld_tile0<MAXS>(a.w_fc, K16, j0, 0, s0, ns, nt, t0w);
        const bool ep = tid < ntl * 64;
        const int row = rb * 16 + er, col = (j0 + et) * 16 + 4 * eq;
        float4 c1 = make_float4(0.f, 0.f, 0.f, 0.f), c2 = c1;
        if (ep) {
            c1 = ld4(a.fc_c1 + col);
            c2 = ld4(a.fc_c2 + col);
        }
        const int n_b = (NCT + a.xt[0] - 1) / a.xt[0];  // attproj units of a row block
        if (!wait6(a, X1 + (has ? rb : 0), has ? n_b : 0, 2, sm)) return;
        PL_MARK(6);
        fs1 = fs2 = 0.f;
        if (has) unit_body<MAXS, true>(a.res2, K16, a.w_fc, K16, rb, 0, j0, ntl, s0, ns, nt, t0w, sm.red, fs1, fs2,
                                       a.layer == 5);
        hpa_gemm::row_sums_publish(fs1, fs2, sm.wsum + w * 32);
        lds_barrier();
        if (ep) {
            float4 v = ln_fold4(sm.wsum, er, C, fold_t<XT_MAX>(sm.red, et, er, eq), c1, c2);
            v = row < a.B ? make_float4(hpa::gelu_ref(v.x), hpa::gelu_ref(v.y), hpa::gelu_ref(v.z), hpa::gelu_ref(v.w))
                          : make_float4(0.f, 0.f, 0.f, 0.f);
            hpa::store_wt16(a.fch, (int)(hpa::frag_index(row, col, 4 * C) * 4), v);
        }
        publish6(a, H + rb * 4, has);
        PL_MARK(7);
    }
    // D: fcproj(l), K part p of 4 (C each): partials -> slab; the last part of
    // (row block, tile group) adds the parts in order + bias + res2 -> res
    {
        const int T = a.xt[2], NG = a.xng[2];
        const int g = bid % NG, q1 = bid / NG, rb = q1 % R, p = q1 / R, j0 = g * T;
        const bool has = p < 4 && j0 < NCT;
        const int ntl = has ? min(T, NCT - j0) : 0;
        if (has) cx::ld_tile0<MAXS>(a.w_fp, 4 * K16, j0, p * K16, s0, ns, nt, t0w);
        const bool ep = tid < ntl * 64;
        const int row = rb * 16 + er, col = (j0 + et) * 16 + 4 * eq;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ep) bv = ld4(a.b_fp + col);
        const int n_c = (4 * NCT + a.xt[1] - 1) / a.xt[1];  // fc units of a row block
        if (!wait6(a, H + (has ? rb * 4 : 0), has ? n_c : 0, 3, sm)) return;
        PL_MARK(8);
        if (has) unit_body<MAXS, false>(a.fch, 4 * K16, a.w_fp, 4 * K16, rb, p * K16, j0, ntl, s0, ns, nt, t0w, sm.red, fs1, fs2);
        lds_barrier();
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        auto slab_at = [&](int pp) { return (((pp * R + rb) * NCT + j0 + et) * 256 + (tid & 63) * 4) * 4; };
        if (ep) {
            val = fold_t<XT_MAX>(sm.red, et, er, eq);
            hpa::store_wt16(a.slab_fp, slab_at(p), val);
        }
        drain_vm();
        lds_barrier();
        if (has && tid == 0) {
            const int tk = __hip_atomic_fetch_add(tick + rb * NG + g, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sm.s_last = tk == 3;
        }
        lds_barrier();
        const bool last = has && sm.s_last != 0;
        if (last && ep) {
            float4 pv[4];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) pv[qq] = qq == p ? val : hpa::load_wt16(a.slab_fp, slab_at(qq));
            const int fi = (int)(hpa::frag_index(row, col, C) * 4);
            const float4 rv = hpa::load_wt16(a.res2, fi);
            float4 tot = pv[0];
#pragma unroll
            for (int qq = 1; qq < 4; ++qq) {
                tot.x += pv[qq].x; tot.y += pv[qq].y; tot.z += pv[qq].z; tot.w += pv[qq].w;
            }
            tot.x += bv.x; tot.y += bv.y; tot.z += bv.z; tot.w += bv.w;
            tot = row < a.B ? make_float4(rv.x + tot.x, rv.y + tot.y, rv.z + tot.z, rv.w + tot.w)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
            hpa::store_wt16(a.res, fi, tot);
            if (a.stats_out) {
                float* tr = sm.tile + (et * 16 + er) * 17 + 4 * eq;
                tr[0] = tot.x; tr[1] = tot.y; tr[2] = tot.z; tr[3] = tot.w;
            }
        }
        drain_vm();
        lds_barrier();
        if (a.stats_out && last && tid < ntl * 16) {  // 16-column LNf partial sums of the tiles' rows
            const int t = tid >> 4, r = tid & 15;
            const float* tr = sm.tile + (t * 16 + r) * 17;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                s1 += tr[c];
                s2 += tr[c] * tr[c];
            }
            const int j = j0 + t, rr = rb * 16 + r;
            a.stats_out[((size_t)j * a.Mp + rr) * 2] = s1;
            a.stats_out[((size_t)j * a.Mp + rr) * 2 + 1] = s2;
        }
        if (tid == 0 && last) arrive6(a, X2 + rb, 1);
        PL_MARK(9);
    }
    // E: qkv(l+1): LN1 folded, q + K/V appended into layer l+1's pages
    if (!a.last) {
        constexpr int NJ = 3 * NCT;
        const int T = a.xt[3], NG = a.xng[3];
        const int g = bid % NG, rb = bid / NG, j0 = g * T;
        const bool has = rb < R && j0 < NJ;
        const int ntl = has ? min(T, NJ - j0) : 0;
        const bool ep = tid < ntl * 64;
        const int row = rb * 16 + er, col = (j0 + et) * 16 + 4 * eq;
        // the K/V destination while the weights stream (as form 6, hpa_chain6.hip qkv_pos6 / qkv_page6)
        const int kps = ep && row < a.B && col >= C ? a.pos[row] : 0;
        if (has) cx::ld_tile0<MAXS>(a.w_qkv, K16, j0, 0, s0, ns, nt, t0w);
        float4 c1 = make_float4(0.f, 0.f, 0.f, 0.f), c2 = c1;
        if (ep) {
            c1 = ld4(a.qkv_c1 + col);
            c2 = ld4(a.qkv_c2 + col);
        }
        const int kpage = ep && row < a.B && col >= C ? a.bt[(size_t)row * a.bt_stride + kps / P] : -1;
        const int n_d = (NCT + a.xt[2] - 1) / a.xt[2];  // fcproj tile groups of a row block
        if (!wait6(a, X2 + (has ? rb : 0), has ? n_d : 0, 4, sm)) return;
        PL_MARK(10);
        fs1 = fs2 = 0.f;
        if (has) unit_body<MAXS, true>(a.res, K16, a.w_qkv, K16, rb, 0, j0, ntl, s0, ns, nt, t0w, sm.red, fs1, fs2);
        hpa_gemm::row_sums_publish(fs1, fs2, sm.wsum + w * 32);
        lds_barrier();
        if (ep && row < a.B) {
            const float4 v = ln_fold4(sm.wsum, er, C, fold_t<XT_MAX>(sm.red, et, er, eq), c1, c2);
            if (col < C) {
                *reinterpret_cast<float4*>(a.q_out + (size_t)row * C + col) = v;
            } else {  // K/V of this token into the sequence's page of layer l+1 (add_to_cache)
                const int kv = col >= 2 * C;
                const int c = col - (kv ? 2 * C : C);
                const int hh = c >> 6, d = c & 63;
                if (kpage >= 0) {
                    const int pslot = kps % P;
                    const size_t toff = hpa::kv_tile_off(kpage, a.page_elems, NH, kv, hh, P);
                    hpa::kv_store4<BF ? 8 : 4>(a.kv_next, toff, kv, d, pslot, P, v);
                }
            }
        }
    }
    PL_MARK(11);
}

// chain form 8: tiles per unit T (<= cx::XT_MAX) and tile groups NG (padded
// to a multiple of 8 where that still fits) of a phase with NJ column tiles
// and `parts` K parts: the fewest tiles with every unit on a workgroup
int pick_xt(int R, int parts, int NJ, int G, int* T, int* NG) {
    for (int pad = 8; pad >= 1; pad /= 8)
        for (int t = (R * parts * NJ + G - 1) / G; t <= cx::XT_MAX; ++t) {
            if (t < 1) continue;
            const int ng = ((NJ + t - 1) / t + pad - 1) / pad * pad;
            if (R * parts * ng <= G) {
                *T = t;
                *NG = ng;
                return 0;
            }
        }
    return 1;
}

}  // namespace

int hpa_chain8_shape(int B, int NH, int G, int xt[4], int xng[4]) {
    const int R = (B + 15) / 16, nct = 4 * NH;  // C / 16
    return B < 1 || B > 64 || pick_xt(R, 1, nct, G, &xt[0], &xng[0]) || pick_xt(R, 1, 4 * nct, G, &xt[1], &xng[1]) ||
           pick_xt(R, 4, nct, G, &xt[2], &xng[2]) || pick_xt(R, 1, 3 * nct, G, &xt[3], &xng[3]);
}

namespace {

template <int NH, int P, bool BF>
int launchx(const HpaLayerArgs* h, int G) {
    HPA_REQUIRE((hpa::resident_blocks<decode_chainx_kernel<NH, P, BF>>(768) >= 1),
                "decode layer: the chain-8 workgroup does not fit a CU");
    KA a;
    fill_ka(h, G, a);
    HPA_REQUIRE(hpa_chain8_shape(h->B, NH, G, a.xt, a.xng) == 0, "decode layer: chain form 8 shape (B <= 64)");
    decode_chainx_kernel<NH, P, BF><<<G, 768, 0, hpa_stream()>>>(a);
    HPA_LAUNCH_CHECK();
    return 0;
}

template <int NH>
int dispatchx(const HpaLayerArgs* h, int G) {
    return hpa::with_page_dtype(h->pool, "decode layer: page size must be 8, 16, 32 or 64", [&](auto p, auto bf) {
        return launchx<NH, decltype(p)::value, decltype(bf)::value>(h, G);
    });
}

}  // namespace

int hpa_chain8_launch(const HpaLayerArgs* h, int G) {
    switch (h->num_heads) {
        case 16: return dispatchx<16>(h, G);
        case 20: return dispatchx<20>(h, G);
        case 25: return dispatchx<25>(h, G);
        default: return dispatchx<12>(h, G);
    }
}

#ifdef HPA_LAYER_TRACE
int hpa_chain8_trace(unsigned long long* host, int layers) {
    return hpa_pl_trace_add(HIP_SYMBOL(g_pl_trace), host, layers);
}
#endif

extern "C" {

// trace build only: form 8's per-wave fc stamps of layer 5 ([256][12][16] u64,
// s_memtime); host NULL clears them.  Returns 1 in the product build.
int hpa_decode_cx_wave_trace(unsigned long long* host) {
#ifdef HPA_LAYER_TRACE
    if (!host) {
        static unsigned long long zero[256 * 12 * 16];
        HPA_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_cx_wave), zero, sizeof(zero)));
        return 0;
    }
    HPA_CHECK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_cx_wave), sizeof(unsigned long long) * 256 * 12 * 16));
    return 0;
#else
    (void)host;
    return 1;
#endif
}

}  // extern "C"
