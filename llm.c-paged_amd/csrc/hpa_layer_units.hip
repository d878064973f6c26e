// hpa_layer_units.hip -- the decode step's layer as ONE persistent launch
// (gfx950), in units of 4 (or 12 / 6) waves: forms 0..5 of hpa_decode_layer,
// of which the product library builds only the 4-wave chain (form 1).
//
// Replaces five launches per layer of the reference layer loop
// (gpt2_forward, paged_infer.c:659-722, one decode row per sequence):
//   A  attention(l)   attention_paged :163-240 (split context, hpa_attn_body.h)
//   B  attproj(l)     matmul_forward :716 + residual_forward :717
//   C  fc(l)          layernorm_forward :718 (folded) + matmul :719 + gelu :720
//   D  fcproj(l)      matmul_forward :721 + residual_forward :722
//   E  qkv(l+1)       layernorm :696 (folded) + matmul_cached :706 + add_to_cache :710
// so a step is embed, qkv(0), L of these, logits, token choice.
//
// Why ("Persistent layer"): every launch of the
// five-kernel layer pays a dispatch + first-round-trip + drain cost, and each
// GEMM starts fetching its weights only after the previous kernel ended.
// Here every phase's weight fragments are loaded into registers before the
// phase's wait, so the weight stream overlaps the hand-off, and the seams
// between phases are in-launch hand-offs.
//
// Geometry: one workgroup of 12 waves per CU (grid = CU count, residency
// checked with the occupancy API), three 4-wave slots.  A phase's units are
// numbered v and dealt v -> (workgroup v % G, slot v / G):
//   A  attention unit (sequence, head, context range; hpa_attn_body.h tiles,
//      folded through LDS by the slot's last wave, split_merge across ranges)
//   B..E  a 16x16 output tile (row block rb, column tile j) over K = C (fc,
//      qkv, attproj) or one of 4 K parts of 4C (fcproj), 4 waves x K/4 each
//      -- the one-shot GEMM kernel's summation order.
// ATTN = false (chain form, the engine's default): no phase A; the attention
// ran as its own launch just before, writing att in frag layout.
// fcproj's K-part partial tiles go to a slab with write-through stores; the
// last part of a tile to draw its ticket sums the parts in part order
// (results independent of arrival order), adds bias and residual.
//
// Hand-offs (hpa_handoff.h): sc1 stores, drain, barrier, one lane adds to the
// phase counter, sharded over 8 lines by workgroup % 8; the consumer's wave 0
// polls every shard, the other waves wait at a barrier.  Counters are zeroed
// before every step (a memset node), one block per layer.  Every spin is
// bounded: on timeout *err gets the phase code and the launch ends.
#include "hpa_layer_common.h"

namespace {
enum { CT_ATT = 0, CT_X1 = 1, CT_H = 2, CT_X2 = 3 };

template <int NH>
struct Smem {
    float red[12 * 256];     // [wave][4 regs][64 lanes] accumulators
    float wsum[12 * 32];     // [wave][16 rows][2] LN row partial sums
    float tile[3 * 16 * 17]; // last layer: [slot][16 rows][17] for the LNf statistics
    float s_m[3][4], s_l[3][4];
    float4 s_acc[3][64];     // [slot][4 waves x 16 lanes] (fp32) / [4 waves x 8 lanes][2] (bf16)
    int s_cnt[3];
    int s_ok;
    int s_last[3];
};

#ifdef HPA_LAYER_TRACE
__device__ unsigned long long g_pl_trace[64][256][16];
#endif

// every thread of the workgroup calls; until the 8 shards of counter `which`
// sum to `expected` (hpa::wait_wg)
template <int NH>
__device__ __forceinline__ bool wait_ctr(const KA& a, int which, int expected, int code, Smem<NH>& sm) {
    return hpa::wait_wg(a.err, a.err_sticky, code, sm.s_ok,
                        [&] { return hpa::shards_reached(a.ctr + which * 8 * kPad, expected); });
}

// one lane, after every storing wave's drain and the workgroup barrier
__device__ __forceinline__ void arrive(const KA& a, int which, int n) {
    hpa::arrive_shard(a.ctr + which * 8 * kPad, n);
}

// ------------------------------------------------------------------ phase A
// attention unit u = (sequence, head) x context range, run by the 4 waves of
// `slot`; the slot folds through LDS with a last-arriving-wave counter (no
// workgroup barrier: the other slots and the staging waves run on)
// q of unit u's (sequence, head) as wave-uniform values (SGPRs): loaded
// before the weight DMA is issued (behind an LDS-DMA the compiler no longer
// proves q unclobbered and would keep it in 64 VGPRs)
template <int NH>
__device__ __forceinline__ void load_q(const KA& a, int u, float (&qv)[HS]) {
    const float4* q4 = reinterpret_cast<const float4*>(a.q + (size_t)(u / a.S) * HS);
#pragma unroll
    for (int i = 0; i < HS / 4; ++i) {
        const float4 t = q4[i];
        qv[4 * i + 0] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.x)));
        qv[4 * i + 1] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.y)));
        qv[4 * i + 2] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.z)));
        qv[4 * i + 3] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.w)));
    }
}

template <int NH, int P, bool BF>
__device__ __forceinline__ void attn_unit(const KA& a, int u, int slot, int wq, Smem<NH>& sm, const float (&qv)[HS]) {
    constexpr int C = LD<NH>::C;
    constexpr int TILE = P * HS;
    constexpr int K = BF ? 2 : 1;    // float4 chunks of the folded state per lane
    constexpr int NL = 16 / K;       // lanes holding it
    const int lane = threadIdx.x & 63;
    const int S = a.S;
    const int bh = u / S;
    const int sr = u - bh * S;
    const int b = bh / NH;
    const int h = bh - b * NH;
    const int ctx = a.pos[b] + 1;
#ifdef HPA_PL_QREG
    const float* qh = qv;
#else
    (void)qv;
    const float* __restrict__ qh = a.q + (size_t)bh * HS;  // scalar loads beside the first page ids
#endif
    const int* bt = a.bt + (size_t)b * a.bt_stride;
    const int n_all = (ctx + 63) >> 6;
    const int it0 = (int)((long long)sr * n_all / S);
    const int it1 = (int)((long long)(sr + 1) * n_all / S);
    float m = a.m_init, l = 0.f;
    float4 acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (BF) {
        const unsigned short* base = reinterpret_cast<const unsigned short*>(a.kv);
        hpa_attn::attn_tiles_bf16<P, 4>(qh, base + (size_t)h * TILE, base + (size_t)(NH + h) * TILE, a.page_elems, bt,
                                        a.bt_stride, ctx, it0, it1, a.qscale, m, l, acc, wq);
#pragma unroll
        for (int o = 8; o <= 32; o <<= 1)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                acc[k].x += __shfl_xor(acc[k].x, o, 64);
                acc[k].y += __shfl_xor(acc[k].y, o, 64);
                acc[k].z += __shfl_xor(acc[k].z, o, 64);
                acc[k].w += __shfl_xor(acc[k].w, o, 64);
            }
    } else {
        const float* base = reinterpret_cast<const float*>(a.kv);
        hpa_attn::attn_tiles<P, 4>(qh, base + (size_t)h * TILE, base + (size_t)(NH + h) * TILE, a.page_elems, bt,
                                   a.bt_stride, ctx, it0, it1, a.qscale, m, l, acc[0], wq);
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            acc[0].x += __shfl_xor(acc[0].x, o, 64);
            acc[0].y += __shfl_xor(acc[0].y, o, 64);
            acc[0].z += __shfl_xor(acc[0].z, o, 64);
            acc[0].w += __shfl_xor(acc[0].w, o, 64);
        }
    }
    l = hpa::wave_sum(l);
    if (lane == 0) {
        sm.s_m[slot][wq] = m;
        sm.s_l[slot][wq] = l;
    }
    if (lane < NL)
#pragma unroll
        for (int k = 0; k < K; ++k) sm.s_acc[slot][(wq * NL + lane) * K + k] = acc[k];
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(&sm.s_cnt[slot], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != 3 || lane >= NL) return;
    // the last wave of the slot: the 4 waves' states in wave order (hpa_attn::attn_fold)
    float M = sm.s_m[slot][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) M = fmaxf(M, sm.s_m[slot][i]);
    float L = 0.f;
    float4 O[K];
#pragma unroll
    for (int k = 0; k < K; ++k) O[k] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float f = exp2f(sm.s_m[slot][i] - M);
        L = fmaf(sm.s_l[slot][i], f, L);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float4 v = sm.s_acc[slot][(i * NL + lane) * K + k];
            O[k].x = fmaf(v.x, f, O[k].x);
            O[k].y = fmaf(v.y, f, O[k].y);
            O[k].z = fmaf(v.z, f, O[k].z);
            O[k].w = fmaf(v.w, f, O[k].w);
        }
    }
    m = M;
    l = L;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = O[k];
    if (S > 1) {
        int* tick = a.ctr + kCtrInts + 2 * a.R * LD<NH>::NCT + bh;  // zeroed per step: no rewind
        if (!hpa_attn::split_merge<K>(a.rec + (size_t)bh * S * kRec, tick, S, sr, m, l, acc, false)) return;
    }
    const float inv = l == 0.f ? 0.f : 1.f / l;
#pragma unroll
    for (int k = 0; k < K; ++k) {  // dims (16/NL)*lane + 4k .. +3 of head h, frag layout
        const int col = h * HS + (64 / NL) * lane + 4 * k;
        hpa::store_wt16(a.att, (int)(hpa::frag_index(b, col, C) * 4),
                        make_float4(acc[k].x * inv, acc[k].y * inv, acc[k].z * inv, acc[k].w * inv));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this (the only storing) wave drained
    if (lane == 0) arrive(a, CT_ATT, 1);
}

// ------------------------------------------------------------------ GEMM units
// A unit is one 16x16 output tile (column tile j, row block rb) over a K range
// of C (the whole K of qkv / attproj / fc, one of 4 parts of fcproj's 4C),
// computed by one 4-wave slot exactly like gemm16_os_kernel<4, *, K16/4>:
// wave wq takes k16 steps [wq*SW, wq*SW+SW), one accumulator chain in k
// order, the 4 waves folded in wave order.  Phase X's units are numbered
// v = (part*R + rb)*NJ + j and dealt v -> workgroup v % G, slot v / G: with
// NJ and G multiples of 8 the row blocks and parts of one weight tile land on
// one XCD (blocks b, b+8 share an XCD) and re-read it from that L2.
// The slot's weight fragments are loaded into registers BEFORE the phase's
// wait (prefetch across the seam); the barriers between phases wait for LDS
// only (lds_barrier), so those loads stay in flight.

struct Unit {
    int j, rb, p;
    bool has;
};
__device__ __forceinline__ Unit unit_of(int v, int n, int NJ, int R) {
    Unit u;
    u.has = v < n;
    const int vv = u.has ? v : 0;
    u.j = vv % NJ;
    const int q = vv / NJ;
    u.rb = q % R;
    u.p = q / R;
    return u;
}

// the wave's weight fragments of column tile j, k16 steps kb + wq*SW ..
// (K16W steps per tile row); non-temporal where one row block reads the tile
template <int SW>
__device__ __forceinline__ void load_w(const float* W, int K16W, int j, int kb, int wq, bool nt, float4 (&wr)[SW]) {
    const float4* wf = reinterpret_cast<const float4*>(W) + ((size_t)j * K16W + kb + wq * SW) * 64 + (threadIdx.x & 63);
    if (nt) {
#pragma unroll
        for (int s = 0; s < SW; ++s) wr[s] = ld_nt(wf + s * 64);
    } else {
#pragma unroll
        for (int s = 0; s < SW; ++s) wr[s] = wf[s * 64];
    }
}

// the wave's A fragments (activation written in this launch: sc1 loads),
// then the one-shot kernel's chain and (STATS) its LN row partial sums
template <int SW, bool STATS>
__device__ __forceinline__ f32x4 unit_mfma(const float* A, int K16A, int rb, int kb, int wq, const float4 (&wr)[SW],
                                           float& fs1, float& fs2) {
    float4 xv[SW];
    const int off = ((rb * K16A + kb + wq * SW) * 64 + (int)(threadIdx.x & 63)) * 16;
#pragma unroll
    for (int s = 0; s < SW; ++s) xv[s] = hpa::load_wt16(A, off + s * 1024);
    __builtin_amdgcn_sched_barrier(0);  // every A load in flight before the first MFMA (see c6::mfma_t)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < SW; ++s) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].x, wr[s].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].y, wr[s].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].z, wr[s].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].w, wr[s].w, acc, 0, 0, 0);
    }
    if (STATS)
#pragma unroll
        for (int s = 0; s < SW; ++s) hpa_gemm::row_sums_add(xv[s], fs1, fs2);
    return acc;
}

__device__ __forceinline__ void put_red(float* red, int wv, f32x4 acc) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int g = 0; g < 4; ++g) red[wv * 256 + g * 64 + lane] = acc[g];
}

// element e = wq*64 + lane of the slot's tile, its 4 waves in wave order
// (Epi<4,...>::finish): row 4*(lane>>4) + wq, column lane & 15
__device__ __forceinline__ float fold4(const float* red, int slot, int e) {
    const float* r = red + slot * 4 * 256 + e;
    float v = r[0];
    v += r[256];
    v += r[512];
    v += r[768];
    return v;
}

// units of NWU waves (unit slot us of the workgroup): the waves in wave order
template <int NWU>
__device__ __forceinline__ float foldn(const float* red, int us, int e) {
    const float* r = red + us * NWU * 256 + e;
    float v = r[0];
#pragma unroll
    for (int w = 1; w < NWU; ++w) v += r[w * 256];
    return v;
}

// unit slots of workgroup bid (UPW per workgroup) that hold one of n units
template <int UPW>
__device__ __forceinline__ int units_with(int bid, int G, int n) {
    int k = 0;
#pragma unroll
    for (int s2 = 0; s2 < UPW; ++s2) k += bid + s2 * G < n;
    return k;
}

// every storing wave drained, then one lane counts the slots that stored
__device__ __forceinline__ void publish(const KA& a, int which, int nslots) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    if (threadIdx.x == 0 && nslots) arrive(a, which, nslots);
}

// ------------------------------------------------------------------ the kernel
// ATTN = false: the chain only (attproj -> fc -> fcproj -> next qkv); the
// attention ran as its own launch just before (hpa_paged_attention_decode_split
// writing `att` in frag layout), so phase B needs no in-launch wait.
// Waves per GEMM unit, per phase (NB attproj, NCD fc and fcproj, NE qkv): 4
// (three 4-wave slots per workgroup), or wide units in the chain form
// (C = 768): 12 (one unit per workgroup, a phase of <= 256 units) or 6 (two
// per workgroup, <= 512 units).  A unit's K range is split over its waves
// (4 * SW / NWU k16 steps each, folded in wave order): with fewer units than
// 4-wave slots the 4-wave form leaves slots idle and runs longer MFMA chains
// per wave
template <int NWU>
struct UW {  // a wave's place in its phase's unit
    int us, wu, v, e, lrow;
    bool fin;
    __device__ __forceinline__ UW(int wv, int bid, int G, int lane) {
        us = wv / NWU;       // unit slot of the workgroup
        wu = wv - us * NWU;  // wave within the unit
        v = bid + us * G;    // the unit slot's unit
        fin = wu < 4;        // the waves that finish the unit's elements
        e = (wu & 3) * 64 + lane;
        lrow = 4 * (lane >> 4) + (wu & 3);
    }
};

template <int NH, int P, bool BF, bool ATTN, int NB, int NCD, int NE>
__global__ __launch_bounds__(768) void decode_layer_kernel(KA args) {
    using D = LD<NH>;
    constexpr int C = D::C, SW = D::SW, NCT = D::NCT;
    static_assert((NB == 4 && NCD == 4 && NE == 4) ||
                      (!ATTN && (SW * 4) % NB == 0 && (SW * 4) % NCD == 0 && (SW * 4) % NE == 0),
                  "wide units: chain form, K split evenly");
    // fields read where used from the kernarg segment (not all hoisted into
    // SGPRs at entry: the attention keeps q in 64 SGPRs)
    const KA& a = *(const KA*)(const void*)__builtin_amdgcn_kernarg_segment_ptr();
    (void)args;
    __shared__ Smem<NH> sm;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = wv >> 2, wq = wv & 3;
    const int lane = threadIdx.x & 63;
    const int bid = blockIdx.x;
    const int R = a.R, G = a.G;
    const int v = bid + slot * G;           // this slot's attention unit (phase A)
    const int lcol = lane & 15;
    const bool nt = R == 1;                 // one row block: every weight tile read once
    PL_STAMP(t_start);
    if (threadIdx.x < 3) sm.s_cnt[threadIdx.x] = 0;
    __syncthreads();

    // A: attention, one unit (sequence, head, context range) per slot
    if constexpr (ATTN) {
        const bool has = v < a.B * NH * a.S;
        float qv[HS];
#ifdef HPA_PL_QREG
        if (has) load_q<NH>(a, v, qv);
#endif
        PL_STAMP(t_issued);
        if (has) attn_unit<NH, P, BF>(a, v, slot, wq, sm, qv);
        PL_MARK(2);
        PL_STORE(1, t_issued);
    }
    PL_STORE(0, t_start);
    float fs1, fs2;
    // B: attproj(l): res2 = res + att . Wap^T + b
    {
        constexpr int SWU = SW * 4 / NB;
        const UW<NB> uw(wv, bid, G, lane);
        const int us = uw.us, wu = uw.wu, e = uw.e, lrow = uw.lrow;
        const bool fin = uw.fin;
        float4 wr[SWU];
        const Unit u = unit_of(uw.v, NCT * R, NCT, R);
        if (u.has) load_w<SWU>(a.w_ap, D::K16, u.j, 0, wu, nt, wr);
        lds_barrier();
        PL_MARK(3);
        if (ATTN && !wait_ctr<NH>(a, CT_ATT, a.B * NH, 1, sm)) return;
        PL_MARK(4);
        const int row = u.rb * 16 + lrow, col = u.j * 16 + lcol;
        const int fi = (int)(hpa::frag_index(row, col, C) * 4);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float bv = 0.f, rv = 0.f;
        if (u.has) {
            if (fin) {
                bv = a.b_ap[col];
                rv = hpa::load_wt4(a.res, fi);
            }
            acc = unit_mfma<SWU, false>(a.att, D::K16, u.rb, 0, wu, wr, fs1, fs2);
        }
        put_red(sm.red, wv, acc);
        lds_barrier();
        if (u.has && fin) {
            float val = foldn<NB>(sm.red, us, e);
            val += bv;
            val = row < a.B ? rv + val : 0.f;  // residual_forward(out, res, proj)
            hpa::store_wt4(a.res2, fi, val);
        }
        publish(a, CT_X1, units_with<12 / NB>(bid, G, NCT * R));
    }
    PL_MARK(5);
    // C: fc(l): fch = gelu(LN2(res2) . Wfc^T + b), LN folded
    {
        constexpr int SWU = SW * 4 / NCD;
        const UW<NCD> uw(wv, bid, G, lane);
        const int us = uw.us, wu = uw.wu, e = uw.e, lrow = uw.lrow;
        const bool fin = uw.fin;
        float4 wr[SWU];
        const Unit u = unit_of(uw.v, 4 * NCT * R, 4 * NCT, R);
        if (u.has) load_w<SWU>(a.w_fc, D::K16, u.j, 0, wu, nt, wr);
        if (!wait_ctr<NH>(a, CT_X1, NCT * R, 2, sm)) return;
        PL_MARK(6);
        const int row = u.rb * 16 + lrow, col = u.j * 16 + lcol;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float c1 = 0.f, c2 = 0.f;
        fs1 = fs2 = 0.f;
        if (u.has) {
            if (fin) {
                c1 = a.fc_c1[col];
                c2 = a.fc_c2[col];
            }
            acc = unit_mfma<SWU, true>(a.res2, D::K16, u.rb, 0, wu, wr, fs1, fs2);
        }
        hpa_gemm::row_sums_publish(fs1, fs2, sm.wsum + wv * 32);
        put_red(sm.red, wv, acc);
        lds_barrier();
        if (u.has && fin) {
            float val = foldn<NCD>(sm.red, us, e);
            val = ln_fold_val<NCD>(sm.wsum, us, lrow, C, val, c1, c2);
            hpa::store_wt4(a.fch, (int)(hpa::frag_index(row, col, 4 * C) * 4), row < a.B ? hpa::gelu_ref(val) : 0.f);
        }
        publish(a, CT_H, units_with<12 / NCD>(bid, G, 4 * NCT * R));
        PL_MARK(7);
    }
    // D: fcproj(l), K part p of 4: partial tiles -> slab; the last part of
    // (rb, j) adds the parts in order + bias + res2 -> res
    {
        constexpr int SWU = SW * 4 / NCD;
        const UW<NCD> uw(wv, bid, G, lane);
        const int us = uw.us, wu = uw.wu, e = uw.e, lrow = uw.lrow;
        const bool fin = uw.fin;
        float4 wr[SWU];
        const Unit u = unit_of(uw.v, NCT * R * D::FP, NCT, R);
        if (u.has) load_w<SWU>(a.w_fp, 4 * D::K16, u.j, u.p * D::K16, wu, nt, wr);
        if (!wait_ctr<NH>(a, CT_H, 4 * NCT * R, 3, sm)) return;
        PL_MARK(8);
        const int row = u.rb * 16 + lrow, col = u.j * 16 + lcol;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (u.has) acc = unit_mfma<SWU, false>(a.fch, 4 * D::K16, u.rb, u.p * D::K16, wu, wr, fs1, fs2);
        put_red(sm.red, wv, acc);
        lds_barrier();
        float val = 0.f;
        const int sofs = ((u.p * R + u.rb) * NCT + u.j) * 256 + e;
        if (u.has && fin) {
            val = foldn<NCD>(sm.red, us, e);
            hpa::store_wt4(a.slab_fp, sofs * 4, val);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        if (u.has && fin && wu == 0 && lane == 0) {
            const int t = __hip_atomic_fetch_add(a.ctr + kCtrInts + R * NCT + u.rb * NCT + u.j, 1, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            sm.s_last[us] = t == D::FP - 1;
        }
        lds_barrier();
        const bool last = u.has && fin && sm.s_last[us] != 0;
        if (last) {
            float pv[D::FP];
#pragma unroll
            for (int q = 0; q < D::FP; ++q)
                pv[q] = q == u.p ? val : hpa::load_wt4(a.slab_fp, (((q * R + u.rb) * NCT + u.j) * 256 + e) * 4);
            const int fi = (int)(hpa::frag_index(row, col, C) * 4);
            const float rv = hpa::load_wt4(a.res2, fi);
            float tot = pv[0];
#pragma unroll
            for (int q = 1; q < D::FP; ++q) tot += pv[q];
            tot += a.b_fp[col];
            tot = row < a.B ? rv + tot : 0.f;
            hpa::store_wt4(a.res, fi, tot);
            if (a.stats_out) sm.tile[(us * 16 + lrow) * 17 + lcol] = tot;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
        if (a.stats_out && wu == 0 && lane < 16 && last) {  // 16-column LNf partial sums of the tile's rows
            const float* tr = sm.tile + (us * 16 + lane) * 17;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                s1 += tr[c];
                s2 += tr[c] * tr[c];
            }
            const int r = u.rb * 16 + lane;
            a.stats_out[((size_t)u.j * a.Mp + r) * 2] = s1;
            a.stats_out[((size_t)u.j * a.Mp + r) * 2 + 1] = s2;
        }
        if (threadIdx.x == 0) {
            int nd = 0;
            for (int s2 = 0; s2 < 12 / NCD; ++s2) nd += sm.s_last[s2] != 0 && bid + s2 * G < NCT * R * D::FP;
            if (nd) arrive(a, CT_X2, nd);
        }
        PL_MARK(9);
    }
    // E: qkv(l+1): LN1 folded, q + K/V appended into layer l+1's pages
    if (!a.last) {
        constexpr int SWU = SW * 4 / NE;
        const UW<NE> uw(wv, bid, G, lane);
        const int us = uw.us, wu = uw.wu, e = uw.e, lrow = uw.lrow;
        const bool fin = uw.fin;
        float4 wr[SWU];
        const Unit u = unit_of(uw.v, 3 * NCT * R, 3 * NCT, R);
        if (u.has) load_w<SWU>(a.w_qkv, D::K16, u.j, 0, wu, nt, wr);
        if (!wait_ctr<NH>(a, CT_X2, NCT * R, 4, sm)) return;
        PL_MARK(10);
        const int row = u.rb * 16 + lrow, col = u.j * 16 + lcol;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float c1 = 0.f, c2 = 0.f;
        fs1 = fs2 = 0.f;
        if (u.has) {
            if (fin) {
                c1 = a.qkv_c1[col];
                c2 = a.qkv_c2[col];
            }
            acc = unit_mfma<SWU, true>(a.res, D::K16, u.rb, 0, wu, wr, fs1, fs2);
        }
        hpa_gemm::row_sums_publish(fs1, fs2, sm.wsum + wv * 32);
        put_red(sm.red, wv, acc);
        lds_barrier();
        if (u.has && fin && row < a.B) {
            float val = foldn<NE>(sm.red, us, e);
            val = ln_fold_val<NE>(sm.wsum, us, lrow, C, val, c1, c2);
            if (col < C) {
                a.q_out[(size_t)row * C + col] = val;
            } else {  // K/V of this token into the sequence's page of layer l+1 (add_to_cache)
                const int kv = col >= 2 * C;
                const int c = col - (kv ? 2 * C : C);
                const int hh = c >> 6, d = c & 63;
                const int ps = a.pos[row];
                const int page = a.bt[(size_t)row * a.bt_stride + ps / P];
                if (page >= 0) {
                    const int pslot = ps % P;
                    const size_t toff = hpa::kv_tile_off(page, a.page_elems, NH, kv, hh, P);
                    hpa::kv_store1_rt(BF ? HPA_BF16 : HPA_F32, a.kv_next, toff, kv, d, pslot, P, val, nullptr, 0);
                }
            }
        }
    }
    PL_MARK(11);
}

template <int NH, int P, bool BF, bool ATTN, int NB = 4, int NCD = 4, int NE = 4>
int launch(const HpaLayerArgs* h, int G) {
    HPA_REQUIRE((hpa::resident_blocks<decode_layer_kernel<NH, P, BF, ATTN, NB, NCD, NE>>(768) >= 1),
                "decode layer: the persistent workgroup does not fit a CU");
#if HPA_ATTN_SWP  // as hpa_attn.hip: 32-bit buffer offsets in the pipelined fp32 tile loop
    HPA_REQUIRE(BF || !ATTN || h->pool->layer_elems * h->pool->elem_bytes < 0x7fffffffull,
                "decode layer (HPA_ATTN_SWP): a layer's pages must be < 2 GiB (32-bit offsets)");
#endif
    KA a;
    fill_ka(h, G, a);
    decode_layer_kernel<NH, P, BF, ATTN, NB, NCD, NE><<<G, 768, 0, hpa_stream()>>>(a);
    HPA_LAUNCH_CHECK();
    return 0;
}

template <int NH, bool ATTN, int NB = 4, int NCD = 4, int NE = 4>
int dispatch_p(const HpaLayerArgs* h, int G) {
    return hpa::with_page_dtype(h->pool, "decode layer: page size must be 8, 16, 32 or 64", [&](auto p, auto bf) {
        return launch<NH, decltype(p)::value, decltype(bf)::value, ATTN, NB, NCD, NE>(h, G);
    });
}

template <int NH>
int dispatch(const HpaLayerArgs* h, int G) {
#ifndef HPA_AB
    // measured slower than the forms the engine picks: in A/B builds only
    if (h->chain_only >= 2)
        return hpa_fail(__FILE__, __LINE__, "decode layer: wide-unit chain forms 2..5 are in A/B builds only (-DHPA_AB)");
    if (!h->chain_only)
        return hpa_fail(__FILE__, __LINE__, "decode layer: the full persistent layer is in A/B builds only (-DHPA_AB)");
    return dispatch_p<NH, false>(h, G);
#else
    if (h->chain_only >= 2) {  // wide units (C = 768), widths (attproj, fc / fcproj, qkv) by chain_only
        if constexpr (LD<NH>::SW % 3 == 0) {
            const int R = (h->B + 15) / 16, nct = LD<NH>::NCT;
            // every phase's units fit its unit slots: attproj R*nct, fc / fcproj 4*R*nct, qkv 3*R*nct
            auto fits = [&](int nb, int ncd, int ne) {
                return R * nct <= 12 / nb * G && 4 * R * nct <= 12 / ncd * G && 3 * R * nct <= 12 / ne * G;
            };
            switch (h->chain_only) {
                case 2:
                    HPA_REQUIRE(fits(12, 12, 12), "decode layer: chain form 2 (12/12/12-wave units) needs B <= 16");
                    return dispatch_p<NH, false, 12, 12, 12>(h, G);
                case 3:
                    HPA_REQUIRE(fits(12, 6, 6), "decode layer: chain form 3 (12/6/6-wave units) needs B <= 32");
                    return dispatch_p<NH, false, 12, 6, 6>(h, G);
                case 4:
                    HPA_REQUIRE(fits(12, 4, 6), "decode layer: chain form 4 (12/4/6-wave units) needs B <= 48");
                    return dispatch_p<NH, false, 12, 4, 6>(h, G);
                case 5:
                    HPA_REQUIRE(fits(12, 4, 4), "decode layer: chain form 5 (12/4/4-wave units) needs B <= 64");
                    return dispatch_p<NH, false, 12, 4, 4>(h, G);
                default:
                    return hpa_fail(__FILE__, __LINE__, "decode layer: chain_only must be 0..6 or 8");
            }
        } else {
            return hpa_fail(__FILE__, __LINE__, "decode layer: wide units need C = 768");
        }
    }
    return h->chain_only ? dispatch_p<NH, false>(h, G) : dispatch_p<NH, true>(h, G);
#endif
}

}  // namespace

int hpa_layer_units_launch(const HpaLayerArgs* h, int G) {
    return h->num_heads == 12 ? dispatch<12>(h, G) : dispatch<2>(h, G);
}

#ifdef HPA_LAYER_TRACE
int hpa_layer_units_trace(unsigned long long* host, int layers) {
    return hpa_pl_trace_add(HIP_SYMBOL(g_pl_trace), host, layers);
}
#endif
