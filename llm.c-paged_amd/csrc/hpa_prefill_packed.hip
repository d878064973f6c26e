// hpa_prefill_packed.hip -- prefill (multi-query) paged attention for bf16 and
// fp8 KV pools on the bf16 matrix pipe (v_mfma_f32_16x16x32_bf16).
//
// The contract is hpa_paged_attention_prefill_ragged's (hpa_prefill.hip).  That
// kernel widens K and V to fp32 before it stages them and multiplies on the
// fp32 MFMA; this one feeds the pools' values to the matrix pipe as the bf16
// values they are (a bf16 code; an e4m3 code decodes to bf16 exactly) and keeps
// the fp32 arithmetic class by splitting the fp32 operands:
//   * q * qscale (fp8: * the head's K scale) and P are cut into three bf16
//     pieces of 8 mantissa bits each (hi = top 16 bits, mid = top 16 bits of
//     x - hi, lo = x - hi - mid: each difference is exact, the pieces sum to x);
//     every piece has its own MFMA into the same fp32 accumulator, so every
//     product is exact and every sum is fp32;
//   * the fp8 V scale multiplies the finished output once.
//
// Workgroup = (sequence, head, 64-query block), 4 waves, wave w owns queries
// 16w .. 16w+15.  Per 32-key tile:
//   * the 256 threads stage the tile as bf16: thread (key = tid & 31, chunk =
//     tid >> 5) takes the 8 dims 8 chunk..+7 of K and of V of its key, one 16-
//     (bf16) or 8-byte (fp8) piece of the pool layout each.  K goes to sK[key]
//     [dim] (rows of 144 B); V goes transposed to sVt[dim][slot(key)] (rows of
//     80 B): the lanes of keys 2i and 2i+1 swap halves so that each stores 4
//     dwords of (key 2i, key 2i+1) pairs.  Slots past the block's last visible
//     key are zero (the pool may hold NaN there; 0 * NaN would poison the
//     accumulator), and their table entries are never read.  Two buffers; the
//     next tile's codes are in registers while this tile computes.
//   * S^T = K Q^T: A = K (row = key lane & 15 of sub-tile u, k = dims 32 kh +
//     8 (lane >> 4)..+7, one 16-byte LDS read), B = a piece of Q (query lane &
//     15, the same dims): 2 sub-tiles x 2 k-halves x 3 pieces.  The C tile gives
//     lane (c = lane & 15, g = lane >> 4) the keys 16u + 4g + r (r = 0..3) of
//     query c: a lane owns one query, so the softmax needs two cross-lane
//     steps (the max over g) and the row sum stays a per-lane partial.
//   * O^T = V^T P^T: the lane's 8 weights are a B operand as they stand, k
//     slot 8g + j holding key 4g + j (j < 4) or 16 + 4g + j - 4: P never goes
//     through LDS.  A = V^T under the same slot order, which is how sVt was
//     written: one 16-byte read per 16-dim tile, 4 tiles x 3 pieces.
// LDS operand reads and the V pair stores are bank-conflict free (row strides
// of 36 and 20 dwords).
#include <math.h>

#include "hpa_internal.h"
#include "hpa_split3.h"

namespace {

constexpr int HS = 64;
constexpr int KT = 32;   // keys per tile
constexpr int QB = 64;   // queries per workgroup
constexpr int KLD = 72;  // sK row: 64 dims + 8 bf16 of padding
constexpr int VLD = 40;  // sVt row: 32 key slots + 8 bf16 of padding
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct PackedArgs {
    const float* q;         // [rows][C] row-major (row = row0[b] + t)
    const void* layer_base;
    size_t page_elems;
    int NH, P, lp;          // lp = log2(P)
    const float* scales;    // fp8 pools: the layer's [2][NH][2] (scale, inv)
    const int* bt;
    int bt_stride;
    const int* start;       // [B] position of row t = 0
    const int* row0;        // [B] first row of sequence b (nullptr: b*T)
    const int* len;         // [B] query rows of sequence b (nullptr: T); T = max
    int T;
    float* out;             // frag layout [Rp][C]
    float qscale, m_init;
};

// two e4m3 codes (bytes 2 hi, 2 hi + 1 of w) as a pair of bf16: the fp32
// decode has 3 mantissa bits, its top 16 bits are the value
template <bool HI>
__device__ __forceinline__ unsigned e4m3x2_to_bf16x2(unsigned w) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
    return (__float_as_uint(f.x) >> 16) | (__float_as_uint(f.y) & 0xffff0000u);
}

// the 8 dims of one staging piece as 4 dwords of bf16 pairs
template <bool FP8>
__device__ __forceinline__ u32x4 piece_bf16(uint4 raw) {
    if constexpr (FP8)
        return u32x4{e4m3x2_to_bf16x2<false>(raw.x), e4m3x2_to_bf16x2<true>(raw.x), e4m3x2_to_bf16x2<false>(raw.y),
                     e4m3x2_to_bf16x2<true>(raw.y)};
    else
        return u32x4{raw.x, raw.y, raw.z, raw.w};
}

// codes of dims 8c..8c+7 of key `key` (<= the block's last visible key): K
// [chunk of 16 B][slot][16 B], V [slot][64]
template <bool FP8>
__device__ __forceinline__ void load_codes(const PackedArgs& a, const int* bt, int h, int key, int c, uint4& k,
                                           uint4& v) {
    const int page = bt[key >> a.lp];
    const int slot = key & (a.P - 1);
    const size_t tile = (size_t)a.P * HS;
    if constexpr (FP8) {
        const unsigned char* base = reinterpret_cast<const unsigned char*>(a.layer_base) + (size_t)page * a.page_elems;
        const uint2 k2 = *reinterpret_cast<const uint2*>(base + (size_t)h * tile + ((size_t)(c >> 1) * a.P + slot) * 16 +
                                                         (c & 1) * 8);
        const uint2 v2 = *reinterpret_cast<const uint2*>(base + (size_t)(a.NH + h) * tile + (size_t)slot * HS + 8 * c);
        k = make_uint4(k2.x, k2.y, 0u, 0u);
        v = make_uint4(v2.x, v2.y, 0u, 0u);
    } else {
        const unsigned short* base = reinterpret_cast<const unsigned short*>(a.layer_base) + (size_t)page * a.page_elems;
        k = *reinterpret_cast<const uint4*>(base + (size_t)h * tile + ((size_t)c * a.P + slot) * 8);
        v = *reinterpret_cast<const uint4*>(base + (size_t)(a.NH + h) * tile + (size_t)slot * HS + 8 * c);
    }
}

// 8 fp32 values -> the three bf16x8 operands of their pieces (hpa_split3.h), here 0 lo, 1 mid, 2 hi
__device__ __forceinline__ void split3x8(const float* x, bf16x8* piece) {
    u32x4 pc[3];
    hpa_split::split3x8(x, pc);
#pragma unroll
    for (int j = 0; j < 3; ++j) piece[2 - j] = __builtin_bit_cast(bf16x8, pc[j]);
}

template <bool FP8>
__global__ __launch_bounds__(256) void prefill_packed_kernel(PackedArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short sK[2][KT * KLD];
    __shared__ __attribute__((aligned(16))) unsigned short sVt[2][HS * VLD];

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
    bf16x8 qB[2][3];
    {
        const int t = min(t0 + c16, Tb - 1);
        const float* qr = a.q + ((size_t)rb0 + t) * C + h * HS + 8 * g;
        const float qs = FP8 ? a.qscale * a.scales[2 * h] : a.qscale;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const float4 x0 = *reinterpret_cast<const float4*>(qr + 32 * kh);
            const float4 x1 = *reinterpret_cast<const float4*>(qr + 32 * kh + 4);
            const float x[8] = {x0.x * qs, x0.y * qs, x0.z * qs, x0.w * qs, x1.x * qs, x1.y * qs, x1.z * qs, x1.w * qs};
            split3x8(x, qB[kh]);
        }
    }
    float m = a.m_init, l = 0.f;  // l: this lane's part of the row sum (keys 16u + 4g + r of every tile)
    f32x4 o[4];                   // O^T tiles: o[dt][r] = dim 16 dt + 4g + r of query c16
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging: thread -> (key skey of the tile, dims 8 sc..+7).  The V pair
    // stores: the lane of the even key keeps dims 8 sc..+3, the odd one
    // 8 sc + 4..+7; vslot = the k slot of the even key in the PV operand order
    const int skey = threadIdx.x & 31, sc = threadIdx.x >> 5;
    const bool odd = skey & 1;
    const int ekey = skey & ~1;
    const int vslot = 8 * ((ekey & 15) >> 2) + 4 * (ekey >> 4) + (ekey & 3);
    const int vrow = 8 * sc + (odd ? 4 : 0);
    uint4 rk, rv;
    bool rin = skey <= kmax;
    load_codes<FP8>(a, bt, h, min(skey, kmax), sc, rk, rv);

    for (int it = 0; it < ntiles; ++it) {
        const int buf = it & 1;
        {
            u32x4 k4 = piece_bf16<FP8>(rk), v4 = piece_bf16<FP8>(rv);
            if (!rin) k4 = v4 = u32x4{0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(&sK[buf][skey * KLD + 8 * sc]) = k4;
            // swap halves with the lane of key skey ^ 1
            const unsigned g0 = __shfl_xor(odd ? v4.x : v4.z, 1, 64), g1 = __shfl_xor(odd ? v4.y : v4.w, 1, 64);
            const unsigned e0 = odd ? g0 : v4.x, e1 = odd ? g1 : v4.y;  // the even key's two dim pairs
            const unsigned o0 = odd ? v4.z : g0, o1 = odd ? v4.w : g1;  // the odd key's
            unsigned* vt = reinterpret_cast<unsigned*>(&sVt[buf][vrow * VLD + vslot]);
            vt[0] = (e0 & 0xffffu) | (o0 << 16);
            vt[VLD / 2] = (e0 >> 16) | (o0 & 0xffff0000u);
            vt[2 * (VLD / 2)] = (e1 & 0xffffu) | (o1 << 16);
            vt[3 * (VLD / 2)] = (e1 >> 16) | (o1 & 0xffff0000u);
        }
        __syncthreads();
        if (it + 1 < ntiles) {
            const int key = (it + 1) * KT + skey;
            rin = key <= kmax;
            load_codes<FP8>(a, bt, h, min(key, kmax), sc, rk, rv);
        }
        const int k0 = it * KT;
        if (k0 <= wave_kmax) {  // any key of the tile visible to this wave's queries
            f32x4 s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kh = 0; kh < 2; ++kh) {
                    const bf16x8 kA = *reinterpret_cast<const bf16x8*>(&sK[buf][(16 * u + c16) * KLD + 32 * kh + 8 * g]);
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc)
                        s[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kA, qB[kh][pc], s[u], 0, 0, 0);
                }
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
            bf16x8 pB[3];
            split3x8(p, pB);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                o[dt] *= alpha;
                const bf16x8 vA = *reinterpret_cast<const bf16x8*>(&sVt[buf][(16 * dt + c16) * VLD + 8 * g]);
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vA, pB[pc], o[dt], 0, 0, 0);
            }
        }
    }
    // the row sum over the 4 lanes g (the same bits in each), normalise, write:
    // o[dt] is 4 consecutive floats of the frag layout
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const int t = t0 + c16;
    if (t < Tb) {
        float inv = l == 0.f ? 0.f : 1.f / l;
        if constexpr (FP8) inv *= a.scales[2 * (NH + h)];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const f32x4 r = o[dt] * inv;
            *reinterpret_cast<f32x4*>(&a.out[hpa::frag_index(rb0 + t, h * HS + 16 * dt + 4 * g, C)]) = r;
        }
    }
}

}  // namespace

extern "C" int hpa_paged_attention_prefill_packed(const float* q, const HpaKVPool* pool, int layer,
                                                  const int* block_table, int bt_stride, const int* start,
                                                  const int* row0, const int* len, int B, int T, float* out_frag) {
    HPA_REQUIRE(pool && pool->base && pool->head_size == HS, "packed prefill attention: pool with head_size 64");
    HPA_REQUIRE(pool->dtype == HPA_BF16 || pool->dtype == HPA_FP8, "packed prefill attention: bf16 or fp8 pool");
    const int P = pool->page_size;
    HPA_REQUIRE(P == 16 || P == 32 || P == 64 || (P == 8 && pool->dtype == HPA_BF16),
                "packed prefill attention: page size 8 (bf16 only), 16, 32 or 64");
    HPA_REQUIRE(pool->dtype != HPA_FP8 || pool->scales, "packed prefill attention: fp8 pool without scales");
    HPA_REQUIRE(layer >= 0 && layer < pool->num_layers, "packed prefill attention: layer out of range");
    HPA_REQUIRE(q && block_table && start && out_frag && B > 0 && T > 0, "packed prefill attention: bad arguments");
    HPA_REQUIRE(!row0 == !len, "packed prefill attention: row0 and len go together");
    PackedArgs a;
    a.q = q;
    a.layer_base = (const char*)pool->base + (size_t)layer * pool->layer_elems * pool->elem_bytes;
    a.page_elems = pool->page_elems;
    a.NH = pool->num_heads;
    a.P = P;
    a.lp = P == 8 ? 3 : P == 16 ? 4 : P == 32 ? 5 : 6;
    a.scales = pool->dtype == HPA_FP8 ? pool->scales + (size_t)layer * 4 * pool->num_heads : nullptr;
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
    const unsigned grid = (unsigned)(B * a.NH * ((T + QB - 1) / QB));
    if (pool->dtype == HPA_FP8)
        prefill_packed_kernel<true><<<grid, 256, 0, hpa_stream()>>>(a);
    else
        prefill_packed_kernel<false><<<grid, 256, 0, hpa_stream()>>>(a);
    HPA_LAUNCH_CHECK();
    return 0;
}
