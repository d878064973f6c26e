// hpa_prefill_split.hip -- prefill (multi-query) paged attention for fp32 KV
// pools on the bf16 matrix pipe (v_mfma_f32_16x16x32_bf16).
//
// The contract is hpa_paged_attention_prefill_ragged's (hpa_prefill.hip), the
// work split hpa_prefill_packed.hip's.  That kernel multiplies pools whose
// values are bf16 already; here all four operands are fp32, so all four are cut
// into three bf16 pieces of 8 mantissa bits each (piece 0 = hi = the top 16
// bits of x, 1 = mid = the top 16 bits of x - hi, 2 = lo = x - hi - mid: each
// difference is exact, the pieces sum to x) and a product a.b is the sum of the
// piece products a_i.b_j with i + j <= 2, each one MFMA into the same fp32
// accumulator.  The three products left out (i + j >= 3) are below 2^-23 |a||b|
// together: one fp32 rounding of the product.  Issue order, smallest first (a
// piece, b piece): (lo, hi) (mid, mid) (hi, lo) | (mid, hi) (hi, mid) | (hi, hi),
// every term over both k-halves before the next.  -DHPA_SPLIT_TERMS=9 (A/B
// builds) puts (lo, lo) (lo, mid) (mid, lo) in front: every product exact.
//
// Workgroup = (sequence, head, 64-query block), 4 waves, wave w owns queries
// 16w .. 16w+15.  Per 32-key tile:
//   * the 256 threads stage the tile: thread (key = tid & 31, chunk = tid >> 5)
//     takes the 8 dims 8 chunk..+7 of K and of V of its key, two 16-byte loads
//     of the fp32 page layout each, and holds them in registers while the
//     current tile computes.  They are split once, at the store: K goes to
//     sK[piece][key][dim] (rows of 144 B), V transposed to sVt[piece][dim]
//     [slot(key)] (rows of 80 B).  For V the lanes of keys 2i and 2i+1 swap four
//     fp32 dims first, so that each then splits 4 dims of both keys and stores
//     one dword (key 2i, key 2i+1) per dim and piece.  Slots past the block's
//     last visible key are zero in every plane (the pool may hold NaN there),
//     their loads go to that key, and their table entries are never read.
//   * S^T = K Q^T: A = a piece of K (row = key lane & 15 of sub-tile u, k = dims
//     32 kh + 8 (lane >> 4)..+7, one 16-byte LDS read per piece), B = a piece of
//     Q (query lane & 15, the same dims): 2 sub-tiles x 2 k-halves x 6 terms.
//     The C tile gives lane (c = lane & 15, g = lane >> 4) the keys 16u + 4g + r
//     (r = 0..3) of query c: a lane owns one query.
//   * O^T = V^T P^T: the lane's 8 weights, split, are B operands as they stand,
//     k slot 8g + j holding key 4g + j (j < 4) or 16 + 4g + j - 4: P never goes
//     through LDS.  A = a piece of V^T under the same slot order: 4 d-tiles x 6
//     terms.
// 48 MFMAs per tile and wave.  One buffer is 3 x (4608 + 5120) B = 29184 B.
// HPA_SPLIT_BUFFERS is an A/B switch: 1 (the default) has two barriers per tile
// and three waves per SIMD, the next tile's loads still in flight under the
// MFMAs; 2 stores the next tile while this one computes (one barrier per tile,
// 58368 B, two waves per SIMD) and took 10 to 42 % longer at every shape
// measured but the two smallest (DESIGN.md "Prefill of fp32 pools on the bf16
// pipe").
#include <math.h>

#include "hpa_internal.h"
#include "hpa_split3.h"

#ifndef HPA_SPLIT_TERMS
#define HPA_SPLIT_TERMS 6
#endif
#ifndef HPA_SPLIT_BUFFERS
#define HPA_SPLIT_BUFFERS 1
#endif

namespace {

constexpr int HS = 64;
constexpr int KT = 32;   // keys per tile
constexpr int QB = 64;   // queries per workgroup
constexpr int KLD = 72;  // sK row: 64 dims + 8 bf16 of padding
constexpr int VLD = 40;  // sVt row: 32 key slots + 8 bf16 of padding
constexpr int NBUF = HPA_SPLIT_BUFFERS;
constexpr int TERM0 = 9 - HPA_SPLIT_TERMS;  // first term issued of the nine below
static_assert((NBUF == 1 || NBUF == 2) && (TERM0 == 0 || TERM0 == 3), "1 or 2 buffers, 6 or 9 terms");
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct SplitArgs {
    const float* q;         // [rows][C] row-major (row = row0[b] + t)
    const float* layer_base;
    size_t page_elems;
    int NH, P, lp;          // lp = log2(P)
    const int* bt;
    int bt_stride;
    const int* start;       // [B] position of row t = 0
    const int* row0;        // [B] first row of sequence b (nullptr: b*T)
    const int* len;         // [B] query rows of sequence b (nullptr: T); T = max
    int T;
    float* out;             // frag layout [Rp][C]
    float qscale, m_init;
};

// dims 8c..8c+7 of key `key` (<= the block's last visible key): K [chunk of 4]
// [slot][4], V [slot][64]
__device__ __forceinline__ void load_kv8(const SplitArgs& a, const int* bt, int h, int key, int c, float* k, float* v) {
    const int page = bt[key >> a.lp];
    const int slot = key & (a.P - 1);
    const size_t tile = (size_t)a.P * HS;
    const float* base = a.layer_base + (size_t)page * a.page_elems;
    const float* kp = base + (size_t)h * tile + ((size_t)(2 * c) * a.P + slot) * 4;
    const float* vp = base + (size_t)(a.NH + h) * tile + (size_t)slot * HS + 8 * c;
    const float4 k0 = *reinterpret_cast<const float4*>(kp), k1 = *reinterpret_cast<const float4*>(kp + (size_t)a.P * 4);
    const float4 v0 = *reinterpret_cast<const float4*>(vp), v1 = *reinterpret_cast<const float4*>(vp + 4);
    k[0] = k0.x, k[1] = k0.y, k[2] = k0.z, k[3] = k0.w, k[4] = k1.x, k[5] = k1.y, k[6] = k1.z, k[7] = k1.w;
    v[0] = v0.x, v[1] = v0.y, v[2] = v0.z, v[3] = v0.w, v[4] = v1.x, v[5] = v1.y, v[6] = v1.z, v[7] = v1.w;
}

using hpa_split::pack_hi16;  // the pieces: hpa_split3.h
using hpa_split::split3;
using hpa_split::split3x8;

__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__global__ __launch_bounds__(256) void prefill_split_kernel(SplitArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short sK[NBUF][3][KT * KLD];
    __shared__ __attribute__((aligned(16))) unsigned short sVt[NBUF][3][HS * VLD];
    // the nine piece products (A piece, B piece), smallest first; TERM0 = 3 leaves out the first three
    constexpr int TA[9] = {2, 2, 1, 2, 1, 0, 1, 0, 0};
    constexpr int TB[9] = {2, 1, 2, 0, 1, 2, 0, 1, 0};

    const int NH = a.NH;
    const int nqb = (a.T + QB - 1) / QB;
    const int qb = blockIdx.x % nqb;
    const int bh = blockIdx.x / nqb;
    const int b = bh / NH, h = bh - b * NH;
    const int Tb = a.len ? a.len[b] : a.T;  // ragged: this sequence's query rows
    if (qb * QB >= Tb) return;              // whole workgroup past them (uniform, before any barrier)
    const int rb0 = a.row0 ? a.row0[b] : b * a.T;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int c16 = lane & 15;
    const int C = NH * HS;
    const int* bt = a.bt + (size_t)b * a.bt_stride;
    const int start = a.start[b];
    const int t0 = qb * QB + 16 * w;  // this wave's first query (row offset in the sequence)
    const int last_t = min(Tb - 1, qb * QB + QB - 1);
    const int kmax = start + last_t;  // last key any query of the block sees
    const int ntiles = kmax / KT + 1;
    const int wave_kmax = t0 < Tb ? start + min(t0 + 15, Tb - 1) : -1;  // -1: a wave with no query row
    const int qpos = start + t0 + c16;                                  // this lane's query position

    // Q operand: query t0 + c16, dims 32 kh + 8g..+7, scaled, in three pieces
    u32x4 qB[2][3];
    {
        const int t = min(t0 + c16, Tb - 1);
        const float* qr = a.q + ((size_t)rb0 + t) * C + h * HS + 8 * g;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const float4 x0 = *reinterpret_cast<const float4*>(qr + 32 * kh);
            const float4 x1 = *reinterpret_cast<const float4*>(qr + 32 * kh + 4);
            const float x[8] = {x0.x * a.qscale, x0.y * a.qscale, x0.z * a.qscale, x0.w * a.qscale,
                                x1.x * a.qscale, x1.y * a.qscale, x1.z * a.qscale, x1.w * a.qscale};
            split3x8(x, qB[kh]);
        }
    }
    float m = a.m_init, l = 0.f;  // l: this lane's part of the row sum (keys 16u + 4g + r of every tile)
    f32x4 o[4];                   // O^T tiles: o[dt][r] = dim 16 dt + 4g + r of query c16
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging: thread -> (key skey of the tile, dims 8 sc..+7).  The V stores:
    // the lane of the even key takes dims 8 sc..+3 of both keys of its pair, the
    // odd one 8 sc + 4..+7; vslot = the k slot of the even key in the PV operand
    // order (even: a dword holds slots vslot, vslot + 1)
    const int skey = threadIdx.x & 31, sc = threadIdx.x >> 5;
    const bool odd = skey & 1;
    const int ekey = skey & ~1;
    const int vslot = 8 * ((ekey & 15) >> 2) + 4 * (ekey >> 4) + (ekey & 3);
    const int vrow = 8 * sc + (odd ? 4 : 0);
    float rk[8], rv[8];
    bool rin = skey <= kmax;
    load_kv8(a, bt, h, min(skey, kmax), sc, rk, rv);

    for (int it = 0; it < ntiles; ++it) {
        const int buf = NBUF == 2 ? it & 1 : 0;
        {
            if (!rin) {
#pragma unroll
                for (int i = 0; i < 8; ++i) rk[i] = rv[i] = 0.f;
            }
            u32x4 k3[3];
            split3x8(rk, k3);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<u32x4*>(&sK[buf][pc][skey * KLD + 8 * sc]) = k3[pc];
            // swap four dims with the lane of key skey ^ 1, then dim vrow + j of (even key, odd key)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float got = __shfl_xor(odd ? rv[j] : rv[4 + j], 1, 64);
                unsigned e[3], d[3];
                split3(odd ? got : rv[j], e);
                split3(odd ? rv[4 + j] : got, d);
#pragma unroll
                for (int pc = 0; pc < 3; ++pc)
                    *reinterpret_cast<unsigned*>(&sVt[buf][pc][(vrow + j) * VLD + vslot]) = pack_hi16(e[pc], d[pc]);
            }
        }
        __syncthreads();
        if (it + 1 < ntiles) {
            const int key = (it + 1) * KT + skey;
            rin = key <= kmax;
            load_kv8(a, bt, h, min(key, kmax), sc, rk, rv);
        }
        const int k0 = it * KT;
        if (k0 <= wave_kmax) {  // any key of the tile visible to this wave's queries
            f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            {
                u32x4 kA[2][2][3];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                        for (int pc = 0; pc < 3; ++pc)
                            kA[u][kh][pc] =
                                *reinterpret_cast<const u32x4*>(&sK[buf][pc][(16 * u + c16) * KLD + 32 * kh + 8 * g]);
#pragma unroll
                for (int t = TERM0; t < 9; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                        for (int u = 0; u < 2; ++u) s[u] = mfma_bf16(kA[u][kh][TA[t]], qB[kh][TB[t]], s[u]);
            }
            // online softmax of query c16 over the lane's 8 keys, the max over the 4 lanes g
            float sv[8];
            float mt = -INFINITY;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int key = k0 + 16 * (i >> 2) + 4 * g + (i & 3);
                sv[i] = key <= qpos ? s[i >> 2][i & 3] : -INFINITY;
                mt = fmaxf(mt, sv[i]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float mn = fmaxf(m, mt);
            const float alpha = exp2f(m - mn);
            float p[8], ps = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                p[i] = exp2f(sv[i] - mn);
                ps += p[i];
            }
            l = fmaf(l, alpha, ps);
            m = mn;
            u32x4 pB[3], vA[4][3];
            split3x8(p, pB);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                o[dt] *= alpha;
#pragma unroll
                for (int pc = 0; pc < 3; ++pc)
                    vA[dt][pc] = *reinterpret_cast<const u32x4*>(&sVt[buf][pc][(16 * dt + c16) * VLD + 8 * g]);
            }
#pragma unroll
            for (int t = TERM0; t < 9; ++t)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt] = mfma_bf16(vA[dt][TA[t]], pB[TB[t]], o[dt]);
        }
        if (NBUF == 1) __syncthreads();  // every wave done with the tile before the next one is stored
    }
    // the row sum over the 4 lanes g (the same bits in each), normalise, write:
    // o[dt] is 4 consecutive floats of the frag layout
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const int t = t0 + c16;
    if (t < Tb) {
        const float inv = l == 0.f ? 0.f : 1.f / l;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const f32x4 r = o[dt] * inv;
            *reinterpret_cast<f32x4*>(&a.out[hpa::frag_index(rb0 + t, h * HS + 16 * dt + 4 * g, C)]) = r;
        }
    }
}

}  // namespace

extern "C" int hpa_paged_attention_prefill_split(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                                 int bt_stride, const int* start, const int* row0, const int* len, int B,
                                                 int T, float* out_frag) {
    HPA_REQUIRE(pool && pool->base && pool->head_size == HS, "split prefill attention: pool with head_size 64");
    HPA_REQUIRE(pool->dtype == HPA_F32, "split prefill attention: fp32 pool");
    const int P = pool->page_size;
    HPA_REQUIRE(P == 8 || P == 16 || P == 32 || P == 64, "split prefill attention: page size 8, 16, 32 or 64");
    HPA_REQUIRE(layer >= 0 && layer < pool->num_layers, "split prefill attention: layer out of range");
    HPA_REQUIRE(q && block_table && start && out_frag && B > 0 && T > 0, "split prefill attention: bad arguments");
    HPA_REQUIRE(!row0 == !len, "split prefill attention: row0 and len go together");
    SplitArgs a;
    a.q = q;
    a.layer_base = (const float*)pool->base + (size_t)layer * pool->layer_elems;
    a.page_elems = pool->page_elems;
    a.NH = pool->num_heads;
    a.P = P;
    a.lp = P == 8 ? 3 : P == 16 ? 4 : P == 32 ? 5 : 6;
    a.bt = block_table;
    a.bt_stride = bt_stride;
    a.start = start;
    a.row0 = row0;
    a.len = len;
    a.T = T;
    a.out = out_frag;
    const float log2e = 1.4426950408889634f;
    a.qscale = (float)(1.0 / sqrt((double)HS)) * log2e;  // the reference's 1/sqrtf(hs), log2 domain
    a.m_init = -10000.0f * log2e;                         // the reference's maxval = -10000
    prefill_split_kernel<<<(unsigned)(B * a.NH * ((T + QB - 1) / QB)), 256, 0, hpa_stream()>>>(a);
    HPA_LAUNCH_CHECK();
    return 0;
}
