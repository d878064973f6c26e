// hpa_verify_packed.hip -- the few-row verify attention on bf16 and fp8 KV
// pools, chain and tree forms, and the tree pass's K/V compaction on them.
//
// The work split is hpa_verify.hip's: one workgroup of NW waves per (sequence,
// head), the context up to the last row's key cut into 64-token tiles, tile
// `it` to wave it % NW, a tile loaded ONCE, non-temporal, straight into
// registers and used for every query row, the queries staged in LDS and read
// by broadcast, R = 2 / 4 / 8 online-softmax states per lane with the row loops
// fully unrolled, the per-wave states folded through LDS in wave order (a
// launch repeats bit for bit), softmax from the -10000 floor.
//
// What the pool layouts change (HpaKVPool, hip_paged_attn.h).  A 16-byte chunk
// holds CH = 8 (bf16) or 16 (fp8) elements, so a 64-token tile is KL = 64 / CH
// = 8 or 4 K loads per lane (lane-per-token: chunk c is dims c CH .. + CH - 1
// of the lane's token) and as many V loads (lane = (g = lane / KL, chunk lane
// % KL): load i is the lane's CH dims of token t0 + CH i + g): 64 or 32 VGPRs
// of codes where an fp32 tile is 128.  A row's state is m, l and CH / 4
// float4.  Codes decode exactly to fp32 (a shift / mask; v_cvt_pk_f32_fp8) and
// every product and sum is fp32 in the decode kernels' order; an fp8 pool's
// per-head scales come from device memory: the finished dot takes qscale *
// k_scale and the finished output v_scale, once.
//
// Decode placement (the template's ONCE).  With 4x .. 8x fewer bytes per tile
// the conversions show, and form (a) -- decode inside each row's loop -- pays
// them R times.  Form (b) turns the loops inside out: chunk outermost, rows
// inside.  One K chunk is decoded into CH registers and dotted into the R
// running scores s[r]; after the R softmax updates one V chunk at a time is
// decoded and added into the R states with the weights p[r].  Every code is
// decoded once per tile, and the decoded tile never exists whole: CH + 2 R
// registers beyond form (a), so the fp8 R = 8 instantiation (144 VGPRs of
// state) has room.  Per row the sums run in the same order in both forms: the
// outputs are bit-identical.  packed_once() names the form the product runs
// per (dtype, R) -- (b) everywhere but bf16 at R = 8 --;
// hpa_set_verify_packed_form picks one for timing tools.
//
// This translation unit is built without packed fp32 VALU forms (Makefile).
#include <math.h>

#include "hpa_attn_body.h"

namespace {
using namespace hpa_attn;

template <int DT>
struct Fmt;
template <>
struct Fmt<HPA_BF16> {
    typedef unsigned short elem;
    static constexpr int CH = 8;
};
template <>
struct Fmt<HPA_FP8> {
    typedef unsigned char elem;
    static constexpr int CH = 16;
};

__device__ __forceinline__ uint4 load_codes(const void* ptr) {
    const hpa::u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const hpa::u32x4*>(ptr));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// form (a): a row's own copy of a chunk of codes.  Left to itself the compiler
// sees R decodes of one value, hoists them out of the rows and holds the whole
// decoded tile (form (b)'s work at several times its registers: the fp8 R = 8
// instantiation spilled to scratch)
__device__ __forceinline__ uint4 row_codes(uint4 u) {
    asm volatile("" : "+v"(u.x), "+v"(u.y), "+v"(u.z), "+v"(u.w));
    return u;
}

// one 16-byte chunk of codes -> its CH exact fp32 values
template <int DT>
__device__ __forceinline__ void decode_chunk(const uint4& u, float (&f)[Fmt<DT>::CH]) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
    if constexpr (DT == HPA_BF16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[2 * j] = bf_lo(w[j]);
            f[2 * j + 1] = bf_hi(w[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 v = hpa::e4m3x4_to_f32(w[j]);
            f[4 * j] = v.x;
            f[4 * j + 1] = v.y;
            f[4 * j + 2] = v.z;
            f[4 * j + 3] = v.w;
        }
    }
}

// s += q[0 .. CH) . k; qc: the chunk's CH / 4 float4 of the row's query in LDS
// (same address in every lane: broadcast)
template <int CH>
__device__ __forceinline__ float dot_chunk(const float4* qc, const float (&k)[CH], float s) {
#pragma unroll
    for (int j = 0; j < CH / 4; ++j) {
        const float4 q4 = qc[j];
        s = fmaf(q4.x, k[4 * j], s);
        s = fmaf(q4.y, k[4 * j + 1], s);
        s = fmaf(q4.z, k[4 * j + 2], s);
        s = fmaf(q4.w, k[4 * j + 3], s);
    }
    return s;
}

template <int CH>
__device__ __forceinline__ void axpy_chunk(float p, const float (&v)[CH], float4 (&a)[CH / 4]) {
#pragma unroll
    for (int j = 0; j < CH / 4; ++j) {
        a[j].x = fmaf(p, v[4 * j], a[j].x);
        a[j].y = fmaf(p, v[4 * j + 1], a[j].y);
        a[j].z = fmaf(p, v[4 * j + 2], a[j].z);
        a[j].w = fmaf(p, v[4 * j + 3], a[j].w);
    }
}

// one tile's scores of one row into its online-softmax state (log2 domain);
// returns the lane's weight p
template <int NA>
__device__ __forceinline__ float softmax_step(float s, float& m, float& l, float4 (&acc)[NA]) {
    const float mt = hpa::wave_max(s);
    const float mn = fmaxf(m, mt);
    const float alpha = exp2f(m - mn);
    const float p = exp2f(s - mn);
    l = fmaf(l, alpha, p);
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        acc[k].x *= alpha;
        acc[k].y *= alpha;
        acc[k].z *= alpha;
        acc[k].w *= alpha;
    }
    m = mn;
    return p;
}

// DT: HPA_BF16 or HPA_FP8.  R: row capacity (len[b] <= R).  TREE: the rows are
// the nodes of a token tree -- node r's K/V sits in slot st + r and row r sees
// the cached keys below st plus slot st + i for every bit i of anc[row] (read
// once per wave ahead of the tile loop, one SGPR per row).  ONCE: form (b)
// above, else form (a).  scales: the fp8 layer's [2][NH][2] (scale, inv).
template <int DT, int P, int NW, int R, bool TREE, bool ONCE>
__global__ __launch_bounds__(NW * 64) void paged_attn_verify_packed(
    const float* __restrict__ q, const void* __restrict__ layer_base, size_t page_elems, int NH,
    const int* __restrict__ block_table, int bt_stride, const int* __restrict__ start,
    const int* __restrict__ row0, const int* __restrict__ len, int T, float* __restrict__ out, float qscale,
    float m_init, const unsigned char* __restrict__ anc, const float* __restrict__ scales) {
    typedef typename Fmt<DT>::elem E;
    constexpr int CH = Fmt<DT>::CH;  // elements per 16-byte chunk; tokens per V load
    constexpr int KL = 64 / CH;      // K loads = V loads per lane and tile; lanes per V row
    constexpr int NA = CH / 4;       // float4 per state
    static_assert(P % CH == 0 && 64 % P == 0, "page size: a multiple of the chunk that divides 64");
    constexpr int TILE = P * HS;
    __shared__ __attribute__((aligned(16))) float s_q[R * HS];
    __shared__ float s_m[R * NW];
    __shared__ float s_l[R * NW];
    __shared__ float4 s_acc[R * NW * 16];

    const int b = (int)blockIdx.x / NH;
    const int h = (int)blockIdx.x - b * NH;
    const int n = min(len ? len[b] : T, R);  // this sequence's query rows
    if (n <= 0) return;                      // whole workgroup (before any barrier)
    const int rb0 = row0 ? row0[b] : b * T;
    const int st = start[b];
    const int ctx = st + n;  // keys of the last row
    const int C = NH * HS;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int g = lane / KL;

    for (int i = threadIdx.x; i < n * HS; i += NW * 64)
        s_q[i] = q[((size_t)rb0 + (i >> 6)) * C + h * HS + (i & 63)];
    __syncthreads();

    float kq = qscale, v_scale = 1.f;
    if constexpr (DT == HPA_FP8) {
        kq = qscale * scales[2 * h];
        v_scale = scales[2 * (NH + h)];
    }
    const E* __restrict__ kbase = reinterpret_cast<const E*>(layer_base) + (size_t)h * TILE;
    const E* __restrict__ vbase = reinterpret_cast<const E*>(layer_base) + (size_t)(NH + h) * TILE;
    const int* bt = block_table + (size_t)b * bt_stride;
    const int it_end = (ctx + 63) >> 6;

    float m[R], l[R];
    float4 acc[R][NA];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        m[r] = m_init;
        l[r] = 0.f;
#pragma unroll
        for (int k = 0; k < NA; ++k) acc[r][k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    unsigned am[R];  // TREE: the rows' ancestor masks, one SGPR each
    if constexpr (TREE) {
        const int mine = lane < n ? (int)anc[rb0 + lane] : 0;
#pragma unroll
        for (int r = 0; r < R; ++r) am[r] = (unsigned)__builtin_amdgcn_readlane(mine, r);
    }

    int it = w;
    int pid = first_tile_pid<P>(bt, bt_stride, ctx, it, it_end);
    for (; it < it_end; it += NW) {
        const unsigned t0 = (unsigned)it << 6;
        const unsigned tok = t0 + lane;
        const E* kt = kbase + (size_t)(unsigned)pid * page_elems + (tok % P) * CH;
        uint4 kv[KL], vv[KL];
#pragma unroll
        for (int c = 0; c < KL; ++c) kv[c] = load_codes(kt + c * P * CH);
        // V load i: tokens t0 + CH i .. + CH - 1 lie in one page (CH <= P, t0 % P == 0):
        // a wave-uniform row address plus a per-lane offset that is the same for every i
#pragma unroll
        for (int i = 0; i < KL; ++i) {
            const int vpid = __builtin_amdgcn_readlane(pid, CH * i);
            const E* vrow = vbase + (size_t)(unsigned)vpid * page_elems + ((CH * i) % P) * HS;
            vv[i] = (t0 + CH * i + g) < (unsigned)ctx ? load_codes(vrow + lane * CH) : make_uint4(0, 0, 0, 0);
        }
        {  // next tile's page ids
            const int itn = it + NW;
            const unsigned t0n = (unsigned)itn << 6, tokn = t0n + lane;
            if (itn < it_end) pid = bt[(tokn < (unsigned)ctx ? tokn : t0n) / P];
        }
        // the queries are re-read from LDS for every tile: an offset the
        // compiler cannot see through keeps the R * 64 loop-invariant values
        // from being hoisted into registers
        int q_off = 0;
        asm volatile("" : "+v"(q_off));
        const float4* qt = reinterpret_cast<const float4*>(s_q + q_off);
        // TREE: this lane's key as a node bit (slot st + i: bit i; a cached key
        // below st or a slot past the nodes: none), once per tile
        unsigned node_bit = 0;
        bool cached = false;
        if constexpr (TREE) {
            const unsigned d = tok - (unsigned)st;  // wraps far above 8 for a cached key
            cached = tok < (unsigned)st;
            node_bit = d < (unsigned)R ? 1u << d : 0u;
        }
        // row r sees keys < st + r + 1: wave-uniform, rows past n and tiles
        // wholly past the row's keys are skipped
        auto live = [&](int r) { return r < n && t0 < (unsigned)(st + r + 1); };
        auto masked = [&](int r, float s) {
            if constexpr (TREE)
                return cached || (node_bit & am[r]) ? s * kq : -INFINITY;
            else
                return tok < (unsigned)(st + r + 1) ? s * kq : -INFINITY;
        };
        if constexpr (ONCE) {
            float s[R], p[R];
#pragma unroll
            for (int r = 0; r < R; ++r) s[r] = p[r] = 0.f;
#pragma unroll
            for (int c = 0; c < KL; ++c) {
                float kf[CH];
                decode_chunk<DT>(kv[c], kf);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (live(r)) s[r] = dot_chunk<CH>(qt + (r * HS + c * CH) / 4, kf, s[r]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (live(r)) p[r] = softmax_step<NA>(masked(r, s[r]), m[r], l[r], acc[r]);
#pragma unroll
            for (int i = 0; i < KL; ++i) {
                float vf[CH];
                decode_chunk<DT>(vv[i], vf);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (live(r)) axpy_chunk<CH>(__shfl(p[r], CH * i + g, 64), vf, acc[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                __builtin_amdgcn_sched_barrier(0);  // one row's reads do not pile up ahead of the row before it
                if (live(r)) {
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < KL; ++c) {
                        float kf[CH];
                        decode_chunk<DT>(row_codes(kv[c]), kf);
                        s = dot_chunk<CH>(qt + (r * HS + c * CH) / 4, kf, s);
                    }
                    const float p = softmax_step<NA>(masked(r, s), m[r], l[r], acc[r]);
#pragma unroll
                    for (int i = 0; i < KL; ++i) {
                        float vf[CH];
                        decode_chunk<DT>(row_codes(vv[i]), vf);
                        axpy_chunk<CH>(__shfl(p, CH * i + g, 64), vf, acc[r]);
                    }
                }
            }
        }
    }

    // fold: the token groups (lane bits above the KL chunk lanes) and the
    // per-lane sums of every wave, then the waves in order through LDS, row r
    // by wave r % NW.  s_acc: [R][NW][KL lanes][NA]
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < n) {
#pragma unroll
            for (int o = KL; o <= 32; o <<= 1)
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    acc[r][k].x += __shfl_xor(acc[r][k].x, o, 64);
                    acc[r][k].y += __shfl_xor(acc[r][k].y, o, 64);
                    acc[r][k].z += __shfl_xor(acc[r][k].z, o, 64);
                    acc[r][k].w += __shfl_xor(acc[r][k].w, o, 64);
                }
            const float lr = hpa::wave_sum(l[r]);
            if (lane == 0) {
                s_m[r * NW + w] = m[r];
                s_l[r * NW + w] = lr;
            }
            if (lane < KL) {
#pragma unroll
                for (int k = 0; k < NA; ++k) s_acc[(r * NW + w) * 16 + lane * NA + k] = acc[r][k];
            }
        }
    }
    __syncthreads();
    if (lane >= KL) return;
    for (int r = w; r < n; r += NW) {
        float M = s_m[r * NW];
#pragma unroll
        for (int i = 1; i < NW; ++i) M = fmaxf(M, s_m[r * NW + i]);
        float L = 0.f;
        float4 O[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) O[k] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const float f = exp2f(s_m[r * NW + i] - M);
            L = fmaf(s_l[r * NW + i], f, L);
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const float4 a = s_acc[(r * NW + i) * 16 + lane * NA + k];
                O[k].x = fmaf(a.x, f, O[k].x);
                O[k].y = fmaf(a.y, f, O[k].y);
                O[k].z = fmaf(a.z, f, O[k].z);
                O[k].w = fmaf(a.w, f, O[k].w);
            }
        }
        const float inv = (L == 0.f ? 0.f : 1.f / L) * v_scale;  // fp8: the raw codes' sum, scaled once
#pragma unroll
        for (int k = 0; k < NA; ++k)  // dims CH lane + 4 k .. + 3
            *reinterpret_cast<float4*>(out + hpa::frag_index(rb0 + r, h * HS + CH * lane + 4 * k, C)) =
                make_float4(O[k].x * inv, O[k].y * inv, O[k].z * inv, O[k].w * inv);
    }
}

struct PackedLaunch {
    const float* q;
    const void* base;
    const float* scales;
    size_t page_elems;
    int NH;
    const int* bt;
    int bt_stride;
    const int *start, *row0, *len;
    int B, T;
    float* out;
    const unsigned char* anc;  // NULL: the chain form
    int nw, form;              // form: 1 (a), 2 (b), 0 the product's pick
};

int g_packed_form = 0;  // hpa_set_verify_packed_form

// the decode placement the product runs per (dtype, rows), as measured
// (profiles/r22/verify_packed.txt, us per launch at B = 64, form a / form b):
// fp8 24.7 / 23.4, 40.4 / 36.1, 93.3 / 91.2 at 2 / 4 / 8 rows; bf16 34.8 / 36.4
// (inside the spread), 45.2 / 42.8, 101.5 / 105.8.  Form (b) but for bf16 at 8
// rows, where the bf16 decode (one shift or mask a value) costs less than
// form (b)'s 16 more live registers.  B = 8 ties throughout.
constexpr bool packed_once(int dt, int R) { return !(dt == HPA_BF16 && R == 8); }

template <int DT, int P, int NW, int R, bool TREE>
void launch_form(const PackedLaunch& a) {
    const float log2e = 1.4426950408889634f;
    const float qscale = (float)(1.0 / sqrt((double)HS)) * log2e;  // as the decode kernel
    const float m_init = -10000.0f * log2e;
    const bool once = a.form ? a.form == 2 : packed_once(DT, R);
    const dim3 grid((unsigned)(a.B * a.NH));
    if (once)
        paged_attn_verify_packed<DT, P, NW, R, TREE, true><<<grid, NW * 64, 0, hpa_stream()>>>(
            a.q, a.base, a.page_elems, a.NH, a.bt, a.bt_stride, a.start, a.row0, a.len, a.T, a.out, qscale, m_init,
            a.anc, a.scales);
    else
        paged_attn_verify_packed<DT, P, NW, R, TREE, false><<<grid, NW * 64, 0, hpa_stream()>>>(
            a.q, a.base, a.page_elems, a.NH, a.bt, a.bt_stride, a.start, a.row0, a.len, a.T, a.out, qscale, m_init,
            a.anc, a.scales);
}

template <int DT, int P, int NW>
void launch_rows(const PackedLaunch& a) {
#define HPA_VP_ROWS(RR) (a.anc ? launch_form<DT, P, NW, RR, true>(a) : launch_form<DT, P, NW, RR, false>(a))
    if (a.T <= 2)
        HPA_VP_ROWS(2);
    else if (a.T <= 4)
        HPA_VP_ROWS(4);
    else
        HPA_VP_ROWS(8);
#undef HPA_VP_ROWS
}

template <int DT, int P>
void launch_page(const PackedLaunch& a) {
    if (a.nw == 8)
        launch_rows<DT, P, 8>(a);
    else
        launch_rows<DT, P, 4>(a);
}

// K/V compaction after a tree pass on a bf16 / fp8 pool
// (hpa_pool_compact_path_packed): hpa_verify.hip's pool_compact_path_kernel
// on the packed layouts.  Grid (sequence, layer); a thread owns fixed 16-byte
// lanes -- (K|V, head, chunk of CH dims) -- of the slot rows and moves, for
// k = 1 .. a in ascending order, its lane of slot start + path[k-1] to slot
// start + k.  In place and safe for the fp32 kernel's reason: path strictly
// increases and path[k-1] >= k.  Bytes only.
constexpr int kCompactThreads = 256;
template <int CH>
__global__ __launch_bounds__(kCompactThreads) void pool_compact_path_packed_kernel(
    unsigned char* __restrict__ base, size_t layer_elems, size_t page_elems, int NH, int P,
    const int* __restrict__ block_table, int bt_stride, const int* __restrict__ start,
    const int* __restrict__ path, const int* __restrict__ n_accepted) {
    constexpr int KL = 64 / CH, EB = 16 / CH;  // chunks per slot row; bytes per element
    const int b = blockIdx.x;
    const int a = min(n_accepted[b], HPA_VERIFY_MAX_ROWS - 1);
    if (a <= 0) return;
    const int st = start[b];
    unsigned char* layer = base + (size_t)blockIdx.y * layer_elems * EB;
    const int* bt = block_table + (size_t)b * bt_stride;
    const int lanes = 2 * NH * KL;
    for (int k = 1; k <= a; ++k) {
        const int src = path[b * HPA_VERIFY_MAX_ROWS + k - 1];
        if (src <= k || src >= HPA_VERIFY_MAX_ROWS) continue;  // in place already (== k), or not a path
        const int ss = st + src, ds = st + k;
        if (ss / P >= bt_stride) continue;
        const int sp = bt[ss / P], dp = bt[ds / P];
        if (sp < 0 || dp < 0) continue;
        for (int i = threadIdx.x; i < lanes; i += kCompactThreads) {
            const int kv = i / (NH * KL), head = (i / KL) % NH, d = (i % KL) * CH;
            const size_t so = hpa::kv_tile_off(sp, page_elems, NH, kv, head, P) +
                              (kv == 0 ? hpa::kv_k_chunk<CH>(d, ss % P, P) : hpa::kv_v_off(d, ss % P));
            const size_t dof = hpa::kv_tile_off(dp, page_elems, NH, kv, head, P) +
                               (kv == 0 ? hpa::kv_k_chunk<CH>(d, ds % P, P) : hpa::kv_v_off(d, ds % P));
            *reinterpret_cast<uint4*>(layer + dof * EB) = *reinterpret_cast<const uint4*>(layer + so * EB);
        }
    }
}

}  // namespace

extern "C" {

int hpa_set_verify_packed_form(int form) {
    HPA_REQUIRE(form >= 0 && form <= 2, "verify packed form: 0 (the product's pick), 1 (a) or 2 (b)");
    g_packed_form = form;
    return 0;
}

int hpa_paged_attention_verify_packed(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                      int bt_stride, const int* start, const int* row0, const int* len,
                                      const unsigned char* anc, int B, int T, float* out_frag) {
    HPA_REQUIRE(pool && pool->base && pool->head_size == HS, "packed verify attention: pool with head_size 64");
    const int P = pool->page_size;
    const bool bf = pool->dtype == HPA_BF16, f8 = pool->dtype == HPA_FP8;
    HPA_REQUIRE(bf || f8, "packed verify attention: bf16 or fp8 pool (fp32 pools: hpa_paged_attention_verify)");
    HPA_REQUIRE(P == 16 || P == 32 || P == 64 || (bf && P == 8),
                "packed verify attention: page size 8 (bf16 only), 16, 32 or 64");
    HPA_REQUIRE(!f8 || pool->scales, "packed verify attention: an fp8 pool needs its scales");
    HPA_REQUIRE(layer >= 0 && layer < pool->num_layers, "packed verify attention: layer out of range");
    HPA_REQUIRE(q && block_table && start && out_frag && B > 0 && bt_stride > 0, "packed verify attention: bad arguments");
    HPA_REQUIRE(T >= 1 && T <= HPA_VERIFY_MAX_ROWS, "packed verify attention: 1..HPA_VERIFY_MAX_ROWS rows per sequence");
    HPA_REQUIRE(!row0 == !len, "packed verify attention: row0 and len go together");
    HPA_REQUIRE(((uintptr_t)out_frag & 15) == 0, "packed verify attention: out must be 16-byte aligned");
    PackedLaunch a;
    a.q = q;
    a.base = (const char*)pool->base + (size_t)layer * pool->layer_elems * pool->elem_bytes;
    a.scales = f8 ? pool->scales + (size_t)layer * 4 * pool->num_heads : nullptr;
    a.page_elems = pool->page_elems;
    a.NH = pool->num_heads;
    a.bt = block_table;
    a.bt_stride = bt_stride;
    a.start = start;
    a.row0 = row0;
    a.len = len;
    a.B = B;
    a.T = T;
    a.out = out_frag;
    a.anc = anc;
    a.form = g_packed_form;
    // 4 or 8 waves: the process-wide override (timing tools, tests) where it names one of them, else by shape
    const int forced = hpa_attention_waves();
    a.nw = forced == 4 || forced == 8 ? forced : hpa_attn_pick_waves(B, pool->num_heads, 1, hpa::num_cus());
    switch (P) {
        case 8: launch_page<HPA_BF16, 8>(a); break;
        case 16: bf ? launch_page<HPA_BF16, 16>(a) : launch_page<HPA_FP8, 16>(a); break;
        case 32: bf ? launch_page<HPA_BF16, 32>(a) : launch_page<HPA_FP8, 32>(a); break;
        default: bf ? launch_page<HPA_BF16, 64>(a) : launch_page<HPA_FP8, 64>(a); break;
    }
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_pool_compact_path_packed(const HpaKVPool* pool, const int* block_table, int bt_stride, const int* start,
                                 const int* path, const int* n_accepted, int B) {
    HPA_REQUIRE(pool && pool->base && block_table && start && path && n_accepted && B > 0 && bt_stride > 0,
                "compact_path_packed: bad arguments");
    HPA_REQUIRE((pool->dtype == HPA_BF16 || pool->dtype == HPA_FP8) && pool->head_size == HS,
                "compact_path_packed: bf16 or fp8 pool with head_size 64 (fp32 pools: hpa_pool_compact_path)");
    HPA_REQUIRE(pool->num_layers <= 65535, "compact_path_packed: too many layers");
    const dim3 grid((unsigned)B, (unsigned)pool->num_layers);
    if (pool->dtype == HPA_BF16)
        pool_compact_path_packed_kernel<8><<<grid, kCompactThreads, 0, hpa_stream()>>>(
            (unsigned char*)pool->base, pool->layer_elems, pool->page_elems, pool->num_heads, pool->page_size,
            block_table, bt_stride, start, path, n_accepted);
    else
        pool_compact_path_packed_kernel<16><<<grid, kCompactThreads, 0, hpa_stream()>>>(
            (unsigned char*)pool->base, pool->layer_elems, pool->page_elems, pool->num_heads, pool->page_size,
            block_table, bt_stride, start, path, n_accepted);
    HPA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
