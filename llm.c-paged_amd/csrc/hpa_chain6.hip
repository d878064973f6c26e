// hpa_chain6.hip -- chain form 6 of hpa_decode_layer (gfx950): the chain
// attproj -> fc -> fcproj -> qkv(l+1) of one layer as one persistent launch of
// multi-tile 12-wave units, and the step's first launch (hpa_decode_first).
// The phases, their reference lines and the hand-off protocol are those of
// hpa_layer_units.hip and hpa_handoff.h.
//
// The default chain form for C = 768.  Every phase runs
// units of all 12 waves of a workgroup (one unit per workgroup): a unit is T
// 16-column tiles of one 16-row block (and, for fcproj, one of its 4 K parts)
// over its K range, wave w taking k16 steps 4w .. 4w+3 of every tile -- the
// summation order of the 12-wave units of chain forms 2..5 (a row's result
// depends on neither T nor the batch, so every batch size and every shard
// computes the same rows).  Against the 4-wave units at B = 64:
//   * a workgroup reads its row block's activation ONCE (48 KB) for its T
//     tiles, where three 4-wave slots read three row blocks (144 KB) through
//     the CU's L2 -> CU path;
//   * the epilogue is 16-byte: a thread owns 4 consecutive columns of one
//     row (one float4 of the next GEMM's frag layout, of q, of a K/V page
//     row), so every hand-off store and residual / bias / LN-fold operand load
//     is dwordx4 (was 4 B per lane);
//   * waits are per row block (fcproj: per row block and K part): a unit
//     waits only for the producers of the rows it reads.
// T per phase (host, dispatch6_t): the fewest tiles with units <= workgroups.
#include "hpa_layer_common.h"

#ifndef HPA_C6_DE
#define HPA_C6_DE 0  // A/B builds: bit 0 fcproj, bit 1 qkv k-group waits at 3-4 row blocks as well
#endif
#ifndef HPA_C6_EARLY
#define HPA_C6_EARLY 0  // A/B builds: 1 = non-storing waves prefetch the next phase's weights right after their MFMAs (measured slower, profiles/r6/experiments/c6_early.txt)
#endif
#ifndef HPA_C6_GW
#define HPA_C6_GW 1  // 1: fc / fcproj / qkv wait per 64-column k-group of their A (wave w on its group); 0: per row block (A/B)
#endif
namespace {
#ifdef HPA_LAYER_TRACE
__device__ unsigned long long g_pl_trace[64][256][16];
#endif

namespace c6 {
using namespace chain;  // NW, the counters X1 / H / X2 / kCtr / kG*, wait6, arrive6, publish6, fold_t, ln_fold4
constexpr int SPW = 4;  // k16 steps per wave of a K = 768 range (48 / 12)
__device__ __forceinline__ void arrive_tiles(const KA& a, int base, int rb, int groups_per_rb, int j0, int n) {
    for (int t = j0; t < j0 + n; ++t)  // tile t of the row block lands in group t / 4
        __hip_atomic_fetch_add(a.ctr + base + (rb * groups_per_rb + t / 4) * kPad, 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

struct Smem6 {
    float red[NW * 3 * 256];  // [wave][tile][256] accumulators
    float wsum[NW * 32];      // [wave][16 rows][2] LN row partial sums
    float tile[3 * 16 * 17];  // last layer: [tile][16 rows][17] for the LNf statistics
    int s_ok;
    int s_last;
    int s_ready;  // HPA_C6_GW: k-groups seen ready by wave 0 (bit 12: the wait failed)
};

// HPA_C6_GW: wave 0 polls the 12 k-group counters of a row block (lane k:
// group k) and publishes the ready set in LDS; wave w goes on as soon as its
// group is in it, so a wave whose producers finished early starts its A loads
// and MFMAs early (the late waves then share the matrix pipe with fewer).
// Bounded like wait6 (hpa::spin_bounded); its own release: no barrier, and a
// failure releases every wave with bit 12 set.
__device__ __forceinline__ bool wait_grp(const KA& a, int base, int expected, int code, Smem6& sm) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    volatile int* rdy = &sm.s_ready;
    if (wv == 0) {
        const int lane = threadIdx.x & 63;
        const bool ok = hpa::spin_bounded(a.err, a.err_sticky, code, [&] {
            const int v = lane < NW ? __hip_atomic_load(a.ctr + base + lane * kPad, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT)
                                    : expected;
            const int m = (int)(__ballot(v >= expected) & 0xFFFull);
            if (lane == 0) *rdy = m;
            return m == 0xFFF;
        });
        if (!ok && lane == 0) *rdy = 0x1FFF;
        return ok;
    }
    int r;
    while (!(((r = *rdy) >> wv) & 1)) __builtin_amdgcn_s_sleep(1);
    return !(r >> 12);
}

// the wave's weight fragments of tiles j0 .. j0+T-1, k16 steps kb + 4w ..
// (NT: non-temporal, one row block reads every tile once; a compile-time
// choice, so the loads carry no branch between them)
template <int T, bool NT>
__device__ __forceinline__ void load_wt(const float* W, int K16W, int j0, int kb, int w, float4 (&wr)[T][SPW]) {
    const float4* wf = reinterpret_cast<const float4*>(W) + ((size_t)j0 * K16W + kb + w * SPW) * 64 + (threadIdx.x & 63);
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int s = 0; s < SPW; ++s) wr[t][s] = NT ? ld_nt(wf + ((size_t)t * K16W + s) * 64) : wf[((size_t)t * K16W + s) * 64];
}

// the wave's 4 A fragments (sc1: written in this launch or the previous
// one), the T tiles' accumulator chains (each in the one-shot order: steps in
// order, components x, y, z, w), and (STATS) the LN row partial sums
template <int T, bool STATS>
__device__ __forceinline__ void mfma_regs(const float4 (&xv)[SPW], const float4 (&wr)[T][SPW], f32x4 (&acc)[T],
                                          float& fs1, float& fs2);

// the wave's 4 A fragments (sc1: written in this launch or the previous one)
__device__ __forceinline__ void load_a4(const float* A, int K16A, int rb, int kb, int w, float4 (&xv)[SPW]) {
    const int off = ((rb * K16A + kb + w * SPW) * 64 + (int)(threadIdx.x & 63)) * 16;
#pragma unroll
    for (int s = 0; s < SPW; ++s) xv[s] = hpa::load_wt16(A, off + s * 1024);
}

template <int T, bool STATS>
__device__ __forceinline__ void mfma_t(const float* A, int K16A, int rb, int kb, int w, const float4 (&wr)[T][SPW],
                                       f32x4 (&acc)[T], float& fs1, float& fs2) {
    float4 xv[SPW];
    const int off = ((rb * K16A + kb + w * SPW) * 64 + (int)(threadIdx.x & 63)) * 16;
#pragma unroll
    for (int s = 0; s < SPW; ++s) xv[s] = hpa::load_wt16(A, off + s * 1024);
    // all four A loads in flight before the first MFMA: left alone the
    // scheduler interleaves them two at a time with the MFMAs (two dependent
    // round trips instead of one, seen in the gfx950 ISA of round 4)
    __builtin_amdgcn_sched_barrier(0);
    mfma_regs<T, STATS>(xv, wr, acc, fs1, fs2);
}

// the T tiles' accumulator chains over the wave's 4 A fragments (each in the
// one-shot order: steps in order, components x, y, z, w) and (STATS) the LN
// row partial sums
template <int T, bool STATS>
__device__ __forceinline__ void mfma_regs(const float4 (&xv)[SPW], const float4 (&wr)[T][SPW], f32x4 (&acc)[T],
                                          float& fs1, float& fs2) {
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < SPW; ++s)
#pragma unroll
        for (int t = 0; t < T; ++t) {
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].x, wr[t][s].x, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].y, wr[t][s].y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].z, wr[t][s].z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].w, wr[t][s].w, acc[t], 0, 0, 0);
        }
    if (STATS)
#pragma unroll
        for (int s = 0; s < SPW; ++s) hpa_gemm::row_sums_add(xv[s], fs1, fs2);
}

template <int T>
__device__ __forceinline__ void put_red_t(float* red, int w, const f32x4 (&acc)[T]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) red[(w * T + t) * 256 + g * 64 + lane] = acc[t][g];
}

// the K / V destination of a qkv epilogue lane, resolved while the unit's
// weights stream and before its wait: the token's position, then its page
// (two dependent loads; issued behind the MFMAs they were the epilogue's
// tail).  qkv_pos6 goes before the weight loads (vmcnt retires in order),
// qkv_page6 after them.
__device__ __forceinline__ int qkv_pos6(const KA& a, bool ep, int row, int col) {
    return ep && row < a.B && col >= 768 ? a.pos[row] : 0;
}
template <int P>
__device__ __forceinline__ int qkv_page6(const KA& a, bool ep, int row, int col, int ps) {
    return ep && row < a.B && col >= 768 ? a.bt[(size_t)row * a.bt_stride + ps / P] : -1;
}

// qkv epilogue store of 4 columns col..col+3 of `row` (NH = 12): q row-major,
// or K / V of this token (position ps, page `page` from qkv_pos6 / qkv_page6)
// into the sequence's page of the layer at kv_next (add_to_cache,
// paged_infer.c:505-573).  An fp8 pool runs the BF = false instantiation and
// branches here on a uniform (kv_scales_next): the four columns become one
// 4-byte store of e4m3fn codes (no third set of chain kernels to build).
template <int P, bool BF>
__device__ __forceinline__ void qkv_store6(const KA& a, int row, int col, int ps, int page, float4 v) {
    constexpr int NH = 12, C = 768;
    if (col < C) {
        *reinterpret_cast<float4*>(a.q_out + (size_t)row * C + col) = v;
        return;
    }
    const int kv = col >= 2 * C;
    const int c = col - (kv ? 2 * C : C);
    const int hh = c >> 6, d = c & 63;
    if (page < 0) return;
    const int pslot = ps % P;
    const size_t toff = hpa::kv_tile_off(page, a.page_elems, NH, kv, hh, P);
    if constexpr (BF) {
        hpa::kv_store4<8>(a.kv_next, toff, kv, d, pslot, P, v);
    } else {
        if (a.kv_scales_next) {  // fp8 pool (pages of 16, 32, 64)
            if constexpr (P % 16 == 0)
                hpa::kv_store4<16>(a.kv_next, toff, kv, d, pslot, P, v, a.kv_scales_next[(kv * NH + hh) * 2 + 1]);
            return;
        }
        hpa::kv_store4<4>(a.kv_next, toff, kv, d, pslot, P, v);
    }
}

}  // namespace c6

// TC, TD, TE: tiles per unit of fc, fcproj, qkv (NH = 12; attproj 1)
template <int P, bool BF, int TC, int TD, int TE>
__global__ __launch_bounds__(768) void decode_chain6_kernel(KA args) {
    using namespace c6;
    constexpr int C = 768, K16 = 48, NCT = 48;
    const KA& a = *(const KA*)(const void*)__builtin_amdgcn_kernarg_segment_ptr();
    (void)args;
    __shared__ Smem6 sm;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = threadIdx.x;
    const int bid = blockIdx.x;
    const int R = a.R;
    constexpr bool NT = TC == 1 && TD == 1 && TE == 1;  // the one-row-block instantiation: every tile read once
    // k-group waits (HPA_C6_GW): fc always; fcproj and qkv at <= 2 row blocks
    // (B <= 32: -1.5 % / -3.3 % per step at B = 32 / 8; at B = 64 they cost
    // what fc's gains, profiles/r4/kgroup_waits.txt)
    constexpr bool GDE = HPA_C6_GW && TC < 3;
    constexpr bool GD = GDE || (HPA_C6_GW != 0 && (HPA_C6_DE & 1) != 0);  // A/B builds: fcproj / qkv k-group waits
    constexpr bool GE = GDE || (HPA_C6_GW != 0 && (HPA_C6_DE & 2) != 0);  // at 3-4 row blocks too
    // epilogue thread's place: tile et, row er, column quad eq
    const int et = tid >> 6, er = (tid & 63) >> 2, eq = tid & 3;
    int* tick = a.ctr + kCtr;  // fcproj K-part tickets [R][NCT / TD]
    if (HPA_C6_GW && tid == 0) sm.s_ready = 0;  // read first in phase C, after phase B's barriers
    PL_STAMP(t_start);
    PL_STORE(0, t_start);
    float fs1 = 0.f, fs2 = 0.f;
    // every phase's unit of this workgroup (the geometry is fixed per launch)
    constexpr int NGB = NCT, NGC = 4 * NCT / TC, NGD = NCT / TD, NGE = 3 * NCT / TE;
    const bool hasB = bid < R * NGB, hasC = bid < R * NGC, hasD = bid < 4 * R * NGD, hasE = bid < R * NGE;
    const int gB = bid % NGB, rbB = bid / NGB;
    const int gC = bid % NGC, rbC = bid / NGC;
    const int gD = bid % NGD, rbD = (bid / NGD) % R, pD = (bid / NGD) / R;
    const int gE = bid % NGE, rbE = bid / NGE;
    // Early weight prefetch (HPA_C6_EARLY, round 6): a wave that stores
    // nothing in phase X (waves >= T_X: only waves 0..T_X-1 run X's epilogue)
    // issues phase X+1's weight fragments (and epilogue operands) right after
    // its MFMAs of phase X (behind their operand waits), so they stream during
    // X's MFMAs, epilogue and seam instead of being issued at the seam, where
    // the A gather after the
    // wait queued behind them in the CU's memory pipe (MI355X_MICROARCH.md
    // "gather-pass": 1.0-1.7 us queued vs 0.3-0.65 quiet).  Such a wave skips
    // the publish drain (it stored nothing; the drain would wait for its
    // prefetch).  The storing waves keep the round-5 order (drain, then the
    // next phase's operands).  Same loads, same arithmetic: same bits.
    constexpr bool EARLY = HPA_C6_EARLY != 0;
    // B: attproj(l), 1 tile per unit: res2 = res + att . Wap^T + b
    float4 c1C = make_float4(0.f, 0.f, 0.f, 0.f), c2C = c1C;
    float4 wrC[TC][SPW];
    {
        constexpr int T = 1;
        const bool has = hasB;
        const int g = gB, rb = rbB;
        float4 wr[T][SPW];
        if (has) load_wt<T, NT>(a.w_ap, K16, g * T, 0, w, wr);
        const bool ep = has && tid < T * 64;
        const int row = rb * 16 + er, col = (g * T + et) * 16 + 4 * eq;
        const int fx = (int)hpa::frag_index(row, col, C), fi = fx * 4;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f), rv = bv;
        if (ep) {
            bv = ld4(a.b_ap + col);
            rv = hpa::load_wt16(a.res, fi);
        }
        PL_MARK(4);
        const bool early = EARLY && w >= T;  // a wave with no store in this phase
        const bool epC = hasC && tid < TC * 64;
        const int colC = (gC * TC + et) * 16 + 4 * eq;
        float4 xv[SPW];
        if (has) load_a4(a.att, K16, rb, 0, w, xv);
        __builtin_amdgcn_sched_barrier(0);
        if (has) {
            f32x4 acc[T];
            mfma_regs<T, false>(xv, wr, acc, fs1, fs2);
            put_red_t<T>(sm.red, w, acc);
        }
        if (early) {  // behind the MFMAs' operand waits (issued here they cannot delay them)
            if (epC) {
                c1C = ld4(a.fc_c1 + colC);
                c2C = ld4(a.fc_c2 + colC);
            }
            if (hasC) load_wt<TC, NT>(a.w_fc, K16, gC * TC, 0, w, wrC);
        }
        lds_barrier();
        if (ep) {
            float4 v = fold_t<T>(sm.red, et, er, eq);
            v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            const bool live = row < a.B;  // residual_forward(out, res, proj); padded rows stay 0
            v = live ? make_float4(rv.x + v.x, rv.y + v.y, rv.z + v.z, rv.w + v.w) : make_float4(0.f, 0.f, 0.f, 0.f);
            hpa::store_wt16(a.res2, fi, v);
        }
        PL_MARK(12);
        if (!early) drain_vm();  // the storing waves
        lds_barrier();
        if (HPA_C6_GW) {  // the tile's k-group of fc's A
            if (tid == 0 && has) arrive_tiles(a, kCtr + 4 * NCT + kGC, rb, NW, g, 1);
        } else {
            if (tid == 0 && has) arrive6(a, X1 + rb, 1);
        }
        if (!early) {  // the round-5 order: epilogue operands, then the weights
            if (epC) {
                c1C = ld4(a.fc_c1 + colC);
                c2C = ld4(a.fc_c2 + colC);
            }
            if (hasC) load_wt<TC, NT>(a.w_fc, K16, gC * TC, 0, w, wrC);
        }
    }
    PL_MARK(5);
    // C: fc(l): fch = gelu(LN2(res2) . Wfc^T + b), LN folded; T = TC tiles
    float4 bvD = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 wrD[TD][SPW];
    {
        constexpr int T = TC;
        const bool has = hasC;
        const int g = gC, rb = rbC;
        const bool ep = has && tid < T * 64;
        const int row = rb * 16 + er, col = (g * T + et) * 16 + 4 * eq;
        if (HPA_C6_GW) {
            if (has && !wait_grp(a, kCtr + 4 * NCT + kGC + rb * NW * kPad, 4, 2, sm)) return;
        } else if (!wait6(a, X1 + (has ? rb : 0), has ? NCT : 0, 2, sm)) {
            return;
        }
        PL_MARK(6);
        const bool early = EARLY && w >= T;
        const bool epD = hasD && tid < TD * 64;
        const int colD = (gD * TD + et) * 16 + 4 * eq;
        fs1 = fs2 = 0.f;
        float4 xv[SPW];
        if (has) load_a4(a.res2, K16, rb, 0, w, xv);
        __builtin_amdgcn_sched_barrier(0);
        if (has) {
            f32x4 acc[T];
            mfma_regs<T, true>(xv, wrC, acc, fs1, fs2);
            put_red_t<T>(sm.red, w, acc);
        }
        hpa_gemm::row_sums_publish(fs1, fs2, sm.wsum + w * 32);
        if (early) {
            if (epD) bvD = ld4(a.b_fp + colD);
            if (hasD) load_wt<TD, NT>(a.w_fp, 4 * K16, gD * TD, pD * K16, w, wrD);
        }
        lds_barrier();
        if (GD && tid == 0) sm.s_ready = 0;  // every wave is past fc's wait; read again in fcproj's
        if (ep) {
            float4 v = ln_fold4(sm.wsum, er, C, fold_t<T>(sm.red, et, er, eq), c1C, c2C);
            const bool live = row < a.B;
            v = live ? make_float4(hpa::gelu_ref(v.x), hpa::gelu_ref(v.y), hpa::gelu_ref(v.z), hpa::gelu_ref(v.w))
                     : make_float4(0.f, 0.f, 0.f, 0.f);
            hpa::store_wt16(a.fch, (int)(hpa::frag_index(row, col, 4 * C) * 4), v);
        }
        PL_MARK(13);
        if (!early) drain_vm();
        lds_barrier();
        if (GD) {  // the tiles' k-groups of fcproj's A (48 per row block)
            if (tid == 0 && has) arrive_tiles(a, kCtr + 4 * NCT + kGD, rb, 4 * NW, g * T, T);
        } else {
            if (tid == 0 && has) arrive6(a, H + rb * 4 + (g * T) / NCT, 1);  // the K part of fcproj these columns feed
        }
        if (!early) {
            if (epD) bvD = ld4(a.b_fp + colD);
            if (hasD) load_wt<TD, NT>(a.w_fp, 4 * K16, gD * TD, pD * K16, w, wrD);
        }
        PL_MARK(7);
    }
    // D: fcproj(l), K part p of 4, T = TD tiles: partial tiles -> slab; the
    // last part of (row block, tile group) adds the parts in order + bias + res2
    float4 wrE[TE][SPW];
    const bool epE = hasE && tid < TE * 64;
    const int rowE = rbE * 16 + er, colE = (gE * TE + et) * 16 + 4 * eq;
    int kps = 0;  // qkv(l+1)'s K/V destination: the row's position (c6::qkv_pos6)
    {
        constexpr int T = TD, NG = NGD;
        const bool has = hasD;
        const int g = gD, rb = rbD, p = pD;
        const bool ep = has && tid < T * 64;
        const int row = rb * 16 + er, col = (g * T + et) * 16 + 4 * eq;
        if (GD) {
            if (has && !wait_grp(a, kCtr + 4 * NCT + kGD + (rb * 4 * NW + p * NW) * kPad, 4, 3, sm)) return;
        } else if (!wait6(a, H + (has ? rb * 4 + p : 0), has ? 4 * NCT / TC / 4 : 0, 3, sm)) {
            return;
        }
        PL_MARK(8);
        const bool early = EARLY && w >= T && !a.last;  // qkv(l+1)'s weights (the storing waves: after the combine)
        float4 xv[SPW];
        if (has) load_a4(a.fch, 4 * K16, rb, p * K16, w, xv);
        __builtin_amdgcn_sched_barrier(0);
        if (has) {
            f32x4 acc[T];
            mfma_regs<T, false>(xv, wrD, acc, fs1, fs2);
            put_red_t<T>(sm.red, w, acc);
        }
        if (early && hasE) load_wt<TE, NT>(a.w_qkv, K16, gE * TE, 0, w, wrE);
        lds_barrier();
        if ((GD || GE) && tid == 0) sm.s_ready = 0;  // every wave is past fcproj's wait; read again in qkv's
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        const int sx = (((p * R + rb) * NG + g) * T * 64 + tid) * 4;  // this part's float4 in the slab (float index)
        if (ep) {
            val = fold_t<T>(sm.red, et, er, eq);
            hpa::store_wt16(a.slab_fp, sx * 4, val);
        }
        PL_MARK(14);
        if (!early) drain_vm();
        lds_barrier();
        if (has && tid == 0) {
            const int tk = __hip_atomic_fetch_add(tick + rb * NG + g, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sm.s_last = tk == 3;
        }
        lds_barrier();
        const bool last = has && sm.s_last != 0;
        if (last && ep) {
            float4 pv[4];
            const int fx = (int)hpa::frag_index(row, col, C), fi = fx * 4;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
                pv[qq] = qq == p ? val : hpa::load_wt16(a.slab_fp, ((((qq * R + rb) * NG + g) * T * 64 + tid) * 4) * 4);
            const float4 rv = hpa::load_wt16(a.res2, fi);
            float4 tot = pv[0];
#pragma unroll
            for (int qq = 1; qq < 4; ++qq) {
                tot.x += pv[qq].x; tot.y += pv[qq].y; tot.z += pv[qq].z; tot.w += pv[qq].w;
            }
            tot.x += bvD.x; tot.y += bvD.y; tot.z += bvD.z; tot.w += bvD.w;
            const bool live = row < a.B;
            tot = live ? make_float4(rv.x + tot.x, rv.y + tot.y, rv.z + tot.z, rv.w + tot.w)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
            hpa::store_wt16(a.res, fi, tot);
            if (a.stats_out) {
                float* tr = sm.tile + (et * 16 + er) * 17 + 4 * eq;
                tr[0] = tot.x; tr[1] = tot.y; tr[2] = tot.z; tr[3] = tot.w;
            }
        }
        if (!early) drain_vm();
        lds_barrier();
        if (a.stats_out && last && tid < T * 16) {  // 16-column LNf partial sums of the tiles' rows
            const int t = tid >> 4, r = tid & 15;
            const float* tr = sm.tile + (t * 16 + r) * 17;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                s1 += tr[c];
                s2 += tr[c] * tr[c];
            }
            const int j = g * T + t, rr = rb * 16 + r;
            a.stats_out[((size_t)j * a.Mp + rr) * 2] = s1;
            a.stats_out[((size_t)j * a.Mp + rr) * 2 + 1] = s2;
        }
        if (tid == 0 && last) {
            if (GE)
                arrive_tiles(a, kCtr + 4 * NCT + kGE, rb, NW, g * T, T);  // the tiles' k-groups of qkv's A
            else
                arrive6(a, X2 + rb, 1);
        }
        PL_MARK(9);
        if (!a.last) {  // the position before the weights (vmcnt retires in order; the page load needs it)
            kps = qkv_pos6(a, epE, rowE, colE);
            if (!early && hasE) load_wt<TE, NT>(a.w_qkv, K16, gE * TE, 0, w, wrE);
        }
    }
    // E: qkv(l+1), T = TE tiles: LN1 folded, q + K/V appended into layer l+1's pages
    if (!a.last) {
        constexpr int T = TE;
        const bool has = hasE;
        const int rb = rbE;
        const bool ep = epE;
        const int row = rowE, col = colE;
        // the epilogue waves' operands (waves 0..TE-1 store in D too: issued
        // after D's drain, as in round 5): the position (above, ahead of the
        // weights), the LN-fold operands, then the page
        float4 c1 = make_float4(0.f, 0.f, 0.f, 0.f), c2 = c1;
        if (ep) {
            c1 = ld4(a.qkv_c1 + col);
            c2 = ld4(a.qkv_c2 + col);
        }
        const int kpage = qkv_page6<P>(a, ep, row, col, kps);
        if (GE) {
            if (has && !wait_grp(a, kCtr + 4 * NCT + kGE + rb * NW * kPad, 4, 4, sm)) return;
        } else if (!wait6(a, X2 + (has ? rb : 0), has ? NCT / TD : 0, 4, sm)) {
            return;
        }
        PL_MARK(10);
        fs1 = fs2 = 0.f;
        if (has) {
            f32x4 acc[T];
            mfma_t<T, true>(a.res, K16, rb, 0, w, wrE, acc, fs1, fs2);
            put_red_t<T>(sm.red, w, acc);
        }
        hpa_gemm::row_sums_publish(fs1, fs2, sm.wsum + w * 32);
        lds_barrier();
        PL_MARK(15);
        if (ep && row < a.B)
            qkv_store6<P, BF>(a, row, col, kps, kpage, ln_fold4(sm.wsum, er, C, fold_t<T>(sm.red, et, er, eq), c1, c2));
    }
    PL_MARK(11);
}


// ------------------------------------------------------------------ the step's first launch (form 6)
// embed (encoder_forward, paged_infer.c:41-47: wte[token] + wpe[pos] at the
// absolute position) and layer 0's qkv in ONE launch, which also zeroes the
// step's counter block and error word: was the embed kernel + the one-shot
// qkv GEMM (two launches and a boundary, 4.3 + 9.4 us at B = 64).  The qkv is
// chain form 6's phase E -- (row block, TE tiles) units, LN1 folded, q + K/V
// of the token into layer 0's pages -- with each wave's A fragments built in
// registers from the embedding instead of loaded; the tile group 0 unit of a
// row block also stores the residual stream it built (frag layout, read by
// layer 0's chain launch).  Rows >= B embed as 0 (padded rows stay 0).
template <int P, bool BF, int TE>
__global__ __launch_bounds__(768) void decode_first6_kernel(KA args) {
    using namespace c6;
    constexpr int C = 768, K16 = 48, NCT = 48;
    const KA& a = *(const KA*)(const void*)__builtin_amdgcn_kernarg_segment_ptr();
    (void)args;
    __shared__ Smem6 sm;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = threadIdx.x, lane = tid & 63;
    const int bid = blockIdx.x;
    constexpr int T = TE, NG = 3 * NCT / TE;
    constexpr bool NT = TE == 1;
    const int g = bid % NG, rb = bid / NG;
    // the row's token and position first: the embedding loads depend on them,
    // and vmcnt retires in order, so behind the weight loads they would wait
    // for those too
    const int arow = rb * 16 + (lane & 15);
    const bool live = rb < a.R && arow < a.B;
    const int tok = live ? a.tokens[arow] : 0, ps = live ? a.pos[arow] : 0;
    for (int i = bid * 768 + tid; i < a.zero_n4; i += (int)gridDim.x * 768) a.zero[i] = make_int4(0, 0, 0, 0);
    if (rb >= a.R) return;  // no unit (the grid holds R * NG <= G of them; nothing here waits)
    const int et = tid >> 6, er = (tid & 63) >> 2, eq = tid & 3;
    const bool ep = tid < T * 64;
    const int row = rb * 16 + er, col = (g * T + et) * 16 + 4 * eq;
    const int kps = qkv_pos6(a, ep, row, col);
    float4 c1 = make_float4(0.f, 0.f, 0.f, 0.f), c2 = c1;
    if (ep) {
        c1 = ld4(a.qkv_c1 + col);
        c2 = ld4(a.qkv_c2 + col);
    }
    float4 wr[T][SPW];
    load_wt<T, NT>(a.w_qkv, K16, g * T, 0, w, wr);
    const int kpage = qkv_page6<P>(a, ep, row, col, kps);
    // A fragment of k16 step 4w + s: lane holds row 16 rb + (lane & 15),
    // columns 16 (4w + s) + 4 (lane >> 4) .. + 3 (hpa::frag_index)
    const float4* te = reinterpret_cast<const float4*>(a.wte + (size_t)tok * C) + (lane >> 4);
    const float4* pe = reinterpret_cast<const float4*>(a.wpe + (size_t)ps * C) + (lane >> 4);
    float4 xv[SPW];
#pragma unroll
    for (int s = 0; s < SPW; ++s) {
        const float4 x = te[(w * SPW + s) * 4], y = pe[(w * SPW + s) * 4];
        xv[s] = live ? make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (g == 0)
#pragma unroll
        for (int s = 0; s < SPW; ++s)
            *reinterpret_cast<float4*>(a.res + ((size_t)(rb * K16 + w * SPW + s) * 64 + lane) * 4) = xv[s];
    float fs1 = 0.f, fs2 = 0.f;
    f32x4 acc[T];
    mfma_regs<T, true>(xv, wr, acc, fs1, fs2);
    put_red_t<T>(sm.red, w, acc);
    hpa_gemm::row_sums_publish(fs1, fs2, sm.wsum + w * 32);
    lds_barrier();
    if (ep && row < a.B)
        qkv_store6<P, BF>(a, row, col, kps, kpage, ln_fold4(sm.wsum, er, C, fold_t<T>(sm.red, et, er, eq), c1, c2));
}

template <int P, bool BF, int TE>
int launch_first6(const HpaLayerArgs* h, int G, const int* tokens, const float* wte, const float* wpe, void* zero,
                  size_t zero_bytes) {
    HPA_REQUIRE((hpa::resident_blocks<decode_first6_kernel<P, BF, TE>>(768) >= 1),
                "decode first: the workgroup does not fit a CU");
    const int R = (h->B + 15) / 16;
    HPA_REQUIRE(R * 144 / TE <= G, "decode first: a unit per workgroup");
    KA a;
    fill_ka(h, G, a);
    a.last = 0;
    a.kv_next = h->pool->base;  // layer 0's pages
    a.kv_scales_next = h->pool->dtype == HPA_FP8 ? h->pool->scales : nullptr;
    a.tokens = tokens;
    a.wte = wte;
    a.wpe = wpe;
    a.zero = reinterpret_cast<int4*>(zero);
    a.zero_n4 = (int)(zero_bytes / 16);
    decode_first6_kernel<P, BF, TE><<<G, 768, 0, hpa_stream()>>>(a);
    HPA_LAUNCH_CHECK();
    return 0;
}

template <int P, bool BF>
int dispatch_first6_t(const HpaLayerArgs* h, int G, const int* tokens, const float* wte, const float* wpe, void* zero,
                      size_t zero_bytes) {
    switch ((h->B + 15) / 16) {  // qkv tiles per unit as chain form 6's phase E
        case 1: return launch_first6<P, BF, 1>(h, G, tokens, wte, wpe, zero, zero_bytes);
        case 2: return launch_first6<P, BF, 2>(h, G, tokens, wte, wpe, zero, zero_bytes);
        case 3: return launch_first6<P, BF, 2>(h, G, tokens, wte, wpe, zero, zero_bytes);
        case 4: return launch_first6<P, BF, 3>(h, G, tokens, wte, wpe, zero, zero_bytes);
        default: return hpa_fail(__FILE__, __LINE__, "decode first: B <= 64");
    }
}

template <int P, bool BF, int TC, int TD, int TE>
int launch6(const HpaLayerArgs* h, int G) {
    HPA_REQUIRE((hpa::resident_blocks<decode_chain6_kernel<P, BF, TC, TD, TE>>(768) >= 1),
                "decode layer: the chain-6 workgroup does not fit a CU");
    const int R = (h->B + 15) / 16;
    HPA_REQUIRE(R * 48 <= G && R * 192 / TC <= G && 4 * R * 48 / TD <= G && R * 144 / TE <= G,
                "decode layer: chain form 6 needs a unit per workgroup in every phase");
    KA a;
    fill_ka(h, G, a);
    decode_chain6_kernel<P, BF, TC, TD, TE><<<G, 768, 0, hpa_stream()>>>(a);
    HPA_LAUNCH_CHECK();
    return 0;
}

// tiles per unit of fc, fcproj, qkv by row blocks R: the fewest with every
// phase's units <= 256 workgroups (attproj: 1)
template <int P, bool BF>
int dispatch6_t(const HpaLayerArgs* h, int G) {
    switch ((h->B + 15) / 16) {
        case 1: return launch6<P, BF, 1, 1, 1>(h, G);
        case 2: return launch6<P, BF, 2, 2, 2>(h, G);
        case 3: return launch6<P, BF, 3, 3, 2>(h, G);
        case 4: return launch6<P, BF, 3, 3, 3>(h, G);
        default: return hpa_fail(__FILE__, __LINE__, "decode layer: chain form 6 needs B <= 64");
    }
}

}  // namespace

int hpa_chain6_launch(const HpaLayerArgs* h, int G) {
    return hpa::with_page_dtype(h->pool, "decode layer: page size must be 8, 16, 32 or 64", [&](auto p, auto bf) {
        return dispatch6_t<decltype(p)::value, decltype(bf)::value>(h, G);
    });
}

#ifdef HPA_LAYER_TRACE
int hpa_chain6_trace(unsigned long long* host, int layers) {
    return hpa_pl_trace_add(HIP_SYMBOL(g_pl_trace), host, layers);
}
#endif

extern "C" {

int hpa_decode_first(const HpaLayerArgs* h, const int* tokens, const float* wte, const float* wpe, void* zero,
                     size_t zero_bytes) {
    HPA_REQUIRE(h && h->pool && h->pool->base && tokens && wte && wpe, "decode first: null operand");
    const HpaKVPool* pool = h->pool;
    HPA_REQUIRE(pool->dtype == HPA_F32 || pool->dtype == HPA_BF16 ||
                    (pool->dtype == HPA_FP8 && pool->scales && pool->page_size % 16 == 0),
                "decode first: fp32, bf16 or fp8 (pages of 16, 32, 64) pool");
    HPA_REQUIRE(h->num_heads == 12 && h->C == 768 && pool->head_size == HS && pool->num_heads == 12,
                "decode first: C = 768, 12 heads of 64");
    HPA_REQUIRE(h->B >= 1 && h->B <= 64, "decode first: 1..64 rows");
    HPA_REQUIRE(h->res && h->w_qkv && h->qkv_c1 && h->qkv_c2 && h->q_out && h->block_table && h->pos,
                "decode first: null operand");
    HPA_REQUIRE(zero_bytes % 16 == 0 && ((size_t)zero & 15) == 0 && zero_bytes / 16 <= 0x7fffffff,
                "decode first: the zeroed block must be whole 16-byte granules");
    const int G = hpa::num_cus();
    return hpa::with_page_dtype(pool, "decode first: page size must be 8, 16, 32 or 64", [&](auto p, auto bf) {
        return dispatch_first6_t<decltype(p)::value, decltype(bf)::value>(h, G, tokens, wte, wpe, zero, zero_bytes);
    });
}

}  // extern "C"
