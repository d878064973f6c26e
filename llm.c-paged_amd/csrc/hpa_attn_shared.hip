// hpa_attn_shared.hip -- decode attention over a shared prefix: the leading
// 64-token tiles that the sequences of a unit hold in the SAME pages
// (gpt2_decode_fork) are streamed once per unit, not once per sequence.
//
// A call is two launches on the current stream; the state crosses the kernel
// boundary in global memory (no in-launch hand-off, ticket or spin):
//  1. prefix: grid (unit, head, prefix split).  The verify kernel's structure
//     (hpa_verify.hip): the unit's tiles [0, unit_tiles) are dealt over the
//     splits and, inside a split, over the NW waves; a tile's K and V rows are
//     loaded once into registers and used for the decode rows of all the
//     unit's <= HPA_SHARED_MAX_ROWS members, whose queries are broadcast from
//     LDS.  Page ids come from the first member's table row (the plan's
//     invariant: every member holds the same pages there) and no key is
//     masked (64 * tiles <= pos of every member).  The waves are folded in
//     wave order and the UNNORMALISED state of (member, head, split) is
//     written as a 68-float record (m, l, -, -, acc[64]) -- the split-context
//     records' layout.  A split without a tile writes the neutral record
//     (m = the floor, l = 0, acc = 0) by the same code path.
//  2. suffix: one workgroup per (sequence, head), the decode kernel's tile
//     loop (attn_tiles) from tile seq_skip[b] on; its final fold takes in b's
//     prefix records in split order ahead of the wave states, normalises and
//     writes out.  With seq_skip[b] == 0 no record is read and the fold is
//     the decode kernel's operation for operation: the row's bits equal
//     hpa_paged_attention_decode_split_w(splits = 1) at the same waves.
// Everything is folded in a fixed order: a call repeats bit for bit.
// Softmax starts from the reference's -10000 floor in every partial state, as
// the waves of the decode kernel do.  fp32 pools, head size 64.
#include <math.h>

#include "hpa_attn_body.h"

// the prefix tiles are read by one workgroup per (unit, head) and, for 9+
// sharers, again by the next unit: -DHPA_SHARED_NT=0 builds load them with the
// default cache policy (profiles/EXPERIMENTS.md)
#ifndef HPA_SHARED_NT
#define HPA_SHARED_NT 1
#endif

namespace {
using namespace hpa_attn;

constexpr int R = HPA_SHARED_MAX_ROWS;

__device__ __forceinline__ float4 load_prefix(const float* ptr) {
#if HPA_SHARED_NT
    return load_stream(ptr);
#else
    return *reinterpret_cast<const float4*>(ptr);
#endif
}

template <int P, int NW>
__global__ __launch_bounds__(NW * 64) void paged_attn_shared_prefix_f32(
    const float* __restrict__ q, const float* __restrict__ layer_base, size_t page_elems, int NH,
    const int* __restrict__ block_table, int bt_stride, const int* __restrict__ pos, int B,
    const int* __restrict__ unit_members, const int* __restrict__ unit_tiles, int S, float* __restrict__ ws,
    float qscale, float m_init) {
    static_assert(P % 4 == 0 && 64 % P == 0, "page size must divide 64 and be a multiple of 4");
    constexpr int TILE = P * HS;
    __shared__ __attribute__((aligned(16))) float s_q[R * HS];
    __shared__ float s_m[R * NW];
    __shared__ float s_l[R * NW];
    __shared__ float4 s_acc[R * NW * 16];

    const int u = (int)blockIdx.x / (NH * S);
    const int hs = (int)blockIdx.x - u * NH * S;
    const int h = hs / S;
    const int sr = hs - h * S;
    int tiles = unit_tiles[u];
    if (tiles <= 0) return;  // unused unit: the whole workgroup, before any barrier
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int d4 = lane & 15;
    const int v_lane_off = g * HS + d4 * 4;

    // the members (wave-uniform): every lane loads entry lane % R, then R readlanes
    int mem[R];
    {
        const int mine = unit_members[u * R + (lane & (R - 1))];
#pragma unroll
        for (int r = 0; r < R; ++r) mem[r] = __builtin_amdgcn_readlane(mine, r);
    }
    int n = 0;  // leading valid members
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (n == r && mem[r] >= 0 && mem[r] < B) n = r + 1;
    if (n == 0) return;
    // never past the first member's keys (0 .. pos) or its table row, whatever the tables hold
    tiles = min(tiles, min((pos[mem[0]] + 1) >> 6, bt_stride * P >> 6));
    const int ctx = tiles << 6;
    const int C = NH * HS;

    for (int i = threadIdx.x; i < n * HS; i += NW * 64) {
        int mr = mem[0];
#pragma unroll
        for (int r = 1; r < R; ++r)
            if ((i >> 6) == r) mr = mem[r];
        s_q[i] = q[(size_t)mr * C + h * HS + (i & 63)];
    }
    __syncthreads();

    const float* __restrict__ kbase = layer_base + (size_t)h * TILE;
    const float* __restrict__ vbase = layer_base + (size_t)(NH + h) * TILE;
    const int* bt = block_table + (size_t)mem[0] * bt_stride;
    const int it_begin = (int)((long long)sr * tiles / S);
    const int it_end = (int)((long long)(sr + 1) * tiles / S);

    float m[R], l[R];
    float4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        m[r] = m_init;
        l[r] = 0.f;
        acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    int it = it_begin + w;
    int pid = first_tile_pid<P>(bt, bt_stride, ctx, it, it_end);
    for (; it < it_end; it += NW) {
        const unsigned t0 = (unsigned)it << 6;
        const unsigned tok = t0 + lane;  // < ctx: whole tiles only
        const float* kt = kbase + (size_t)(unsigned)pid * page_elems + (tok % P) * 4;
        float4 kv[16], vv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) kv[c] = load_prefix(kt + c * P * 4);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int vpid = __builtin_amdgcn_readlane(pid, 4 * i);
            const float* vrow = vbase + (size_t)(unsigned)vpid * page_elems + ((4 * i) % P) * HS;
            vv[i] = load_prefix(vrow + v_lane_off);
        }
        {  // next tile's page ids
            const int itn = it + NW;
            if (itn < it_end) pid = bt[(((unsigned)itn << 6) + lane) / P];
        }
        // the queries are re-read from LDS for every tile, behind an offset the
        // compiler cannot see through (as the verify kernel: hoisted they would spill)
        int q_off = 0;
        asm volatile("" : "+v"(q_off));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            __builtin_amdgcn_sched_barrier(0);
            // t0 < ctx always holds; it keeps the test loop-variant: on r < n alone the compiler
            // unswitches the tile loop by member count and its copies need 258 VGPRs (scratch)
            if (r < n && t0 < (unsigned)ctx) {
                const float4* qr = reinterpret_cast<const float4*>(s_q + q_off + r * HS);
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const float4 q4 = qr[c];  // same address in every lane: broadcast
                    s = fmaf(q4.x, kv[c].x, s);
                    s = fmaf(q4.y, kv[c].y, s);
                    s = fmaf(q4.z, kv[c].z, s);
                    s = fmaf(q4.w, kv[c].w, s);
                }
                s *= qscale;
                const float mt = hpa::wave_max(s);
                const float mn = fmaxf(m[r], mt);
                const float alpha = exp2f(m[r] - mn);
                const float p = exp2f(s - mn);
                l[r] = fmaf(l[r], alpha, p);
                acc[r].x *= alpha;
                acc[r].y *= alpha;
                acc[r].z *= alpha;
                acc[r].w *= alpha;
                m[r] = mn;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float pi = __shfl(p, 4 * i + g, 64);
                    acc[r].x = fmaf(pi, vv[i].x, acc[r].x);
                    acc[r].y = fmaf(pi, vv[i].y, acc[r].y);
                    acc[r].z = fmaf(pi, vv[i].z, acc[r].z);
                    acc[r].w = fmaf(pi, vv[i].w, acc[r].w);
                }
            }
        }
    }

    // fold: the 4 token groups and the per-lane sums of every wave, then the
    // waves in order through LDS, row r by wave r % NW; the record stays unnormalised
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < n) {
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                acc[r].x += __shfl_xor(acc[r].x, o, 64);
                acc[r].y += __shfl_xor(acc[r].y, o, 64);
                acc[r].z += __shfl_xor(acc[r].z, o, 64);
                acc[r].w += __shfl_xor(acc[r].w, o, 64);
            }
            const float lr = hpa::wave_sum(l[r]);
            if (lane == 0) {
                s_m[r * NW + w] = m[r];
                s_l[r * NW + w] = lr;
            }
            if (lane < 16) s_acc[(r * NW + w) * 16 + lane] = acc[r];
        }
    }
    __syncthreads();
    if (lane >= 16) return;
    for (int r = w; r < n; r += NW) {
        float M = s_m[r * NW];
#pragma unroll
        for (int i = 1; i < NW; ++i) M = fmaxf(M, s_m[r * NW + i]);
        float L = 0.f;
        float4 O = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const float f = exp2f(s_m[r * NW + i] - M);
            L = fmaf(s_l[r * NW + i], f, L);
            const float4 a = s_acc[(r * NW + i) * 16 + lane];
            O.x = fmaf(a.x, f, O.x);
            O.y = fmaf(a.y, f, O.y);
            O.z = fmaf(a.z, f, O.z);
            O.w = fmaf(a.w, f, O.w);
        }
        int mr = mem[0];
#pragma unroll
        for (int k = 1; k < R; ++k)
            if (k == r) mr = mem[k];
        float* rec = ws + (((size_t)mr * NH + h) * S + sr) * kRec;
        if (lane == 0) *reinterpret_cast<float4*>(rec) = make_float4(M, L, 0.f, 0.f);
        *reinterpret_cast<float4*>(rec + 4 + 4 * lane) = O;
    }
}

// The decode kernel's fold (attn_fold) with b's np prefix records taken in
// ahead of the wave states.  np == 0: attn_fold's operations in attn_fold's
// order (the same bits).
template <int NW>
__device__ __forceinline__ bool fold_with_prefix(float& m, float& l, float4& acc, float* s_m, float* s_l,
                                                 float4* s_acc, const float* __restrict__ rec, int np) {
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        acc.x += __shfl_xor(acc.x, o, 64);
        acc.y += __shfl_xor(acc.y, o, 64);
        acc.z += __shfl_xor(acc.z, o, 64);
        acc.w += __shfl_xor(acc.w, o, 64);
    }
    l = hpa::wave_sum(l);
    if constexpr (NW == 1) {
        if (lane >= 16) return false;
        if (np == 0) return true;
        s_m[0] = m;  // one wave: its own lanes read these back, in program order
        s_l[0] = l;
        s_acc[lane] = acc;
    } else {
        if (lane == 0) {
            s_m[w] = m;
            s_l[w] = l;
        }
        if (lane < 16) s_acc[w * 16 + lane] = acc;
        __syncthreads();
        if (w != 0 || lane >= 16) return false;
    }
    float M = s_m[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) M = fmaxf(M, s_m[i]);
    for (int s = 0; s < np; ++s) M = fmaxf(M, rec[(size_t)s * kRec]);
    float L = 0.f;
    float4 O = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < np; ++s) {  // the prefix splits, in split order
        const float* rs = rec + (size_t)s * kRec;
        const float f = exp2f(rs[0] - M);
        L = fmaf(rs[1], f, L);
        const float4 a = *reinterpret_cast<const float4*>(rs + 4 + 4 * lane);
        O.x = fmaf(a.x, f, O.x);
        O.y = fmaf(a.y, f, O.y);
        O.z = fmaf(a.z, f, O.z);
        O.w = fmaf(a.w, f, O.w);
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const float f = exp2f(s_m[i] - M);
        L = fmaf(s_l[i], f, L);
        const float4 a = s_acc[i * 16 + lane];
        O.x = fmaf(a.x, f, O.x);
        O.y = fmaf(a.y, f, O.y);
        O.z = fmaf(a.z, f, O.z);
        O.w = fmaf(a.w, f, O.w);
    }
    m = M;
    l = L;
    acc = O;
    return true;
}

template <int P, int NW, bool FRAG>
__global__ __launch_bounds__(NW * 64, 3) void paged_attn_shared_suffix_f32(
    const float* __restrict__ q, const float* __restrict__ layer_base, size_t page_elems, int NH,
    const int* __restrict__ block_table, int bt_stride, const int* __restrict__ pos,
    const int* __restrict__ seq_skip, float* __restrict__ out, float qscale, float m_init, int S,
    const float* __restrict__ ws) {
    constexpr int TILE = P * HS;
    __shared__ float s_m[NW];
    __shared__ float s_l[NW];
    __shared__ float4 s_acc[NW * 16];

    const int bh = (int)blockIdx.x;
    const int b = bh / NH;
    const int h = bh - b * NH;
    const int lane = threadIdx.x & 63;
    const int ctx = pos[b] + 1;
    const float* __restrict__ qh = q + ((size_t)b * NH + h) * HS;  // scalar loads, as the decode kernel
    const int* bt = block_table + (size_t)b * bt_stride;
    const int n_it = (ctx + 63) >> 6;
    const int skip = min(max(seq_skip[b], 0), n_it);  // the tiles b's unit has streamed (wave-uniform)
    float m = m_init;
    float l = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    attn_tiles<P, NW>(qh, layer_base + (size_t)h * TILE, layer_base + (size_t)(NH + h) * TILE, page_elems, bt,
                      bt_stride, ctx, skip, n_it, qscale, m, l, acc);
    const float* rec = ws + (size_t)bh * S * kRec;  // dereferenced only where skip > 0
    if (!fold_with_prefix<NW>(m, l, acc, s_m, s_l, s_acc, rec, skip > 0 && ws ? S : 0)) return;
    const size_t oi = FRAG ? hpa::frag_index(b, h * HS + 4 * lane, NH * HS) : ((size_t)b * NH + h) * HS + 4 * lane;
    const float inv = l == 0.f ? 0.f : 1.f / l;
    *reinterpret_cast<float4*>(out + oi) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
}

struct SharedLaunch {
    const float* q;
    const float* base;
    size_t page_elems;
    int NH;
    const int* bt;
    int bt_stride;
    const int* pos;
    float* out;
    int B;
    const int *members, *tiles, *skip;
    int max_units, S;
    float* ws;
    float qscale, m_init;
};

template <int P, int NW>
void launch_prefix(const SharedLaunch& a) {
    paged_attn_shared_prefix_f32<P, NW><<<(unsigned)(a.max_units * a.NH * a.S), NW * 64, 0, hpa_stream()>>>(
        a.q, a.base, a.page_elems, a.NH, a.bt, a.bt_stride, a.pos, a.B, a.members, a.tiles, a.S, a.ws, a.qscale,
        a.m_init);
}

template <int P, int NW, bool FRAG>
void launch_suffix(const SharedLaunch& a) {
    paged_attn_shared_suffix_f32<P, NW, FRAG><<<(unsigned)(a.B * a.NH), NW * 64, 0, hpa_stream()>>>(
        a.q, a.base, a.page_elems, a.NH, a.bt, a.bt_stride, a.pos, a.skip, a.out, a.qscale, a.m_init, a.S, a.ws);
}

template <int P, bool FRAG>
void launch_suffix_waves(const SharedLaunch& a, int nw) {
    switch (nw) {
        case 1: launch_suffix<P, 1, FRAG>(a); break;
        case 2: launch_suffix<P, 2, FRAG>(a); break;
        case 8: launch_suffix<P, 8, FRAG>(a); break;
        default: launch_suffix<P, 4, FRAG>(a); break;
    }
}

template <int P>
int launch_shared(const SharedLaunch& a, int nw, bool frag) {
    if (a.max_units > 0) {  // the prefix deals tiles over 4 or 8 waves
        if (nw == 8)
            launch_prefix<P, 8>(a);
        else
            launch_prefix<P, 4>(a);
        HPA_LAUNCH_CHECK();
    }
    if (frag)
        launch_suffix_waves<P, true>(a, nw);
    else
        launch_suffix_waves<P, false>(a, nw);
    HPA_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t hpa_attn_shared_ws_bytes(int B, int num_heads, int prefix_splits) {
    if (B <= 0 || num_heads <= 0 || prefix_splits < 1) return 0;
    return (size_t)B * num_heads * prefix_splits * kRec * sizeof(float);
}

// The prefix launch's ranges, a power of two: enough that units * heads *
// ranges reach two workgroups per CU (a few units still fill the device), but
// no more than leave a range about three tiles (a 4-wave workgroup with fewer
// has idle waves and the launch more records to merge).  Measured at 15 tiles
// (profiles/r16/shared_attention.txt, us per launch at 1 / 2 / 4 / 8 / 16
// ranges): 8 units 44.3 / 29.2 / 26.1 / 35.8 / 52.8, 32 units 42.3 / 40.9 /
// 44.2 / 55.3 / 78.2, 1 unit 29.5 / 22.3 / 20.0 / 20.5 / 23.8 -- the rule picks
// 4, 2 and 4.
int hpa_attn_shared_pick_splits(int units, int num_heads, int max_tiles, int num_cus) {
    if (units <= 0 || num_heads <= 0 || max_tiles <= 0) return 1;
    if (num_cus <= 0) num_cus = 256;
    int s = 1;
    while (s < HPA_ATTN_MAX_SPLITS && (long)units * num_heads * s < 2L * num_cus && (s * 2) * 3 <= max_tiles) s *= 2;
    return s;
}

int hpa_paged_attention_decode_shared(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                      int bt_stride, const int* pos, float* out, int B, const int* unit_members,
                                      const int* unit_tiles, int max_units, const int* seq_skip, int prefix_splits,
                                      void* ws, int out_frag, int waves) {
    HPA_REQUIRE(pool && pool->base, "shared attention: pool not created");
    HPA_REQUIRE(pool->dtype == HPA_F32, "shared attention: fp32 pool");
    HPA_REQUIRE(pool->head_size == HS, "shared attention: head_size 64");
    HPA_REQUIRE(pool->page_size == 8 || pool->page_size == 16 || pool->page_size == 32 || pool->page_size == 64,
                "shared attention: page size must be 8, 16, 32 or 64");
    HPA_REQUIRE(layer >= 0 && layer < pool->num_layers, "shared attention: layer out of range");
    HPA_REQUIRE(B > 0 && bt_stride > 0 && q && out && block_table && pos && seq_skip, "shared attention: bad arguments");
    HPA_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)out & 15) == 0, "shared attention: q/out must be 16-byte aligned");
    HPA_REQUIRE(prefix_splits >= 1 && prefix_splits <= HPA_ATTN_MAX_SPLITS,
                "shared attention: prefix_splits 1..HPA_ATTN_MAX_SPLITS");
    HPA_REQUIRE(max_units >= 0 && (max_units == 0 || (unit_members && unit_tiles)),
                "shared attention: unit tables");
    HPA_REQUIRE(max_units == 0 || (ws && ((uintptr_t)ws & 15) == 0),
                "shared attention: a 16-byte aligned workspace (hpa_attn_shared_ws_bytes) while a unit exists");
    HPA_REQUIRE(waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8, "attention waves 1, 2, 4, 8");
    const int forced = hpa_attention_waves();
    const int nw = forced ? forced : waves ? waves : 4;
    const float log2e = 1.4426950408889634f;
    SharedLaunch a;
    a.q = q;
    a.base = (const float*)pool->base + (size_t)layer * pool->layer_elems;
    a.page_elems = pool->page_elems;
    a.NH = pool->num_heads;
    a.bt = block_table;
    a.bt_stride = bt_stride;
    a.pos = pos;
    a.out = out;
    a.B = B;
    a.members = unit_members;
    a.tiles = unit_tiles;
    a.skip = seq_skip;
    a.max_units = max_units;
    a.S = prefix_splits;
    a.ws = (float*)ws;
    a.qscale = (float)(1.0 / sqrt((double)HS)) * log2e;  // as the decode kernel
    a.m_init = -10000.0f * log2e;
    switch (pool->page_size) {
        case 8: return launch_shared<8>(a, nw, out_frag != 0);
        case 16: return launch_shared<16>(a, nw, out_frag != 0);
        case 32: return launch_shared<32>(a, nw, out_frag != 0);
        default: return launch_shared<64>(a, nw, out_frag != 0);
    }
}

}  // extern "C"
