// hpa_verify.hip -- speculative greedy decoding on the device: the few-row
// attention of a verify pass, the pass's row tables and the accept decision.
//
// A verify pass runs T = 1 + (drafts) <= HPA_VERIFY_MAX_ROWS query rows per
// sequence over that sequence's whole cached context: row t at position
// start + t sees keys 0 .. start + t.  The shape is a decode step's (a long
// K/V stream per (sequence, head), a handful of queries), not a prompt's, so
// the kernel is the decode kernel's structure (hpa_attn.hip, hpa_attn_body.h)
// with the query dimension added:
//  * one workgroup of NW waves per (sequence, head); the context up to the
//    last row's key is cut into 64-token tiles, tile `it` goes to wave it % NW;
//  * a tile's K rows (lane-per-token, 16 float4 per lane) and V rows
//    (lane-per-dimension, 16 float4 per lane) are loaded ONCE, non-temporal,
//    straight into registers, and used for every query row of the sequence:
//    the launch streams what one decode launch streams;
//  * the queries do not fit SGPRs (8 rows x 64 floats against ~100 SGPRs):
//    the workgroup stages its rows' 64 dims in LDS once and every lane reads
//    them at the same address (a broadcast ds_read_b128, no bank conflict);
//  * row t masks keys past start + t: only the last tile or two differ
//    between rows, and a tile wholly past a row's keys is skipped for that row;
//  * R sets of online-softmax state (m, l, acc) per lane (R = 2, 4 or 8, the
//    template's row capacity: 6 VGPRs each), the loops over rows fully
//    unrolled so every state stays in registers (no scratch);
//  * the per-wave states are folded through LDS in wave order, row r by wave
//    r % NW: a launch repeats bit for bit.
// Softmax starts from the reference's -10000 floor exactly like the decode
// and prefill kernels (a row whose scores all lie far below it gives 0).
// fp32 pools only: bf16 and fp8 pools take hpa_paged_attention_prefill_ragged
// (gpt2_decode_verify_plan).  No context splits.
#include <math.h>

#include "hpa_attn_body.h"

namespace {
using namespace hpa_attn;

// R: row capacity (len[b] <= R).  TREE: the rows are the nodes of a token
// tree (hpa_paged_attention_verify_tree): node r's K/V sits in slot st + r and
// row r sees the cached keys below st plus slot st + i for every bit i of its
// ancestor mask anc[row] (its own bit is the highest, so ctx_r = st + r + 1
// still bounds its tiles).  The masks are wave-uniform: each wave reads its
// sequence's <= 8 bytes once, ahead of the tile loop, and keeps them in SGPRs.
template <int P, int NW, int R, bool TREE>
__global__ __launch_bounds__(NW * 64) void paged_attn_verify_f32(
    const float* __restrict__ q, const float* __restrict__ layer_base, size_t page_elems, int NH,
    const int* __restrict__ block_table, int bt_stride, const int* __restrict__ start,
    const int* __restrict__ row0, const int* __restrict__ len, int T, float* __restrict__ out, float qscale,
    float m_init, const unsigned char* __restrict__ anc) {
    static_assert(P % 4 == 0 && 64 % P == 0, "page size must divide 64 and be a multiple of 4");
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
    const int g = lane >> 4;
    const int d4 = lane & 15;
    const int v_lane_off = g * HS + d4 * 4;

    for (int i = threadIdx.x; i < n * HS; i += NW * 64)
        s_q[i] = q[((size_t)rb0 + (i >> 6)) * C + h * HS + (i & 63)];
    __syncthreads();

    const float* __restrict__ kbase = layer_base + (size_t)h * TILE;
    const float* __restrict__ vbase = layer_base + (size_t)(NH + h) * TILE;
    const int* bt = block_table + (size_t)b * bt_stride;
    const int it_end = (ctx + 63) >> 6;

    float m[R], l[R];
    float4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        m[r] = m_init;
        l[r] = 0.f;
        acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
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
        const float* kt = kbase + (size_t)(unsigned)pid * page_elems + (tok % P) * 4;
        float4 kv[16], vv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) kv[c] = load_stream(kt + c * P * 4);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int vpid = __builtin_amdgcn_readlane(pid, 4 * i);
            const float* vrow = vbase + (size_t)(unsigned)vpid * page_elems + ((4 * i) % P) * HS;
            vv[i] = (t0 + 4 * i + g) < (unsigned)ctx ? load_stream(vrow + v_lane_off)
                                                     : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        {  // next tile's page ids
            const int itn = it + NW;
            const unsigned t0n = (unsigned)itn << 6, tokn = t0n + lane;
            if (itn < it_end) pid = bt[(tokn < (unsigned)ctx ? tokn : t0n) / P];
        }
        // the queries are re-read from LDS for every tile: an offset the
        // compiler cannot see through keeps the R * 64 loop-invariant values
        // from being hoisted into registers (they would spill), and the
        // scheduling barrier keeps one row's reads from piling up ahead of
        // the row before it
        int q_off = 0;
        asm volatile("" : "+v"(q_off));
        // TREE: this lane's key as a node bit (slot st + i: bit i; a cached key
        // below st or a slot past the nodes: none), once per tile
        unsigned node_bit = 0;
        bool cached = false;
        if constexpr (TREE) {
            const unsigned d = tok - (unsigned)st;  // wraps far above 8 for a cached key
            cached = tok < (unsigned)st;
            node_bit = d < (unsigned)R ? 1u << d : 0u;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // row r sees keys < st + r + 1 (wave-uniform: rows past n, tiles past the row's keys)
            const unsigned ctx_r = (unsigned)(st + r + 1);
            __builtin_amdgcn_sched_barrier(0);
            if (r < n && t0 < ctx_r) {
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
                if constexpr (TREE) {
                    s = cached || (node_bit & am[r]) ? s * qscale : -INFINITY;
                } else {
                    s = tok < ctx_r ? s * qscale : -INFINITY;
                }
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
    // waves in order through LDS, row r by wave r % NW
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
        const float inv = L == 0.f ? 0.f : 1.f / L;
        *reinterpret_cast<float4*>(out + hpa::frag_index(rb0 + r, h * HS + 4 * lane, C)) =
            make_float4(O.x * inv, O.y * inv, O.z * inv, O.w * inv);
    }
}

struct VerifyLaunch {
    const float* q;
    const float* base;
    size_t page_elems;
    int NH;
    const int* bt;
    int bt_stride;
    const int *start, *row0, *len;
    int B, T;
    float* out;
    const unsigned char* anc;  // tree form only
};

template <int P, int NW, int R, bool TREE>
void launch_rows(const VerifyLaunch& a) {
    const float log2e = 1.4426950408889634f;
    const float qscale = (float)(1.0 / sqrt((double)HS)) * log2e;  // as the decode kernel
    const float m_init = -10000.0f * log2e;
    paged_attn_verify_f32<P, NW, R, TREE><<<(unsigned)(a.B * a.NH), NW * 64, 0, hpa_stream()>>>(
        a.q, a.base, a.page_elems, a.NH, a.bt, a.bt_stride, a.start, a.row0, a.len, a.T, a.out, qscale, m_init,
        a.anc);
}

template <int P, int NW, bool TREE>
void launch_waves(const VerifyLaunch& a) {
    if (a.T <= 2)
        launch_rows<P, NW, 2, TREE>(a);
    else if (a.T <= 4)
        launch_rows<P, NW, 4, TREE>(a);
    else
        launch_rows<P, NW, 8, TREE>(a);
}

template <int P, bool TREE>
void launch_page(const VerifyLaunch& a, int nw) {
    if (nw == 8)
        launch_waves<P, 8, TREE>(a);
    else
        launch_waves<P, 4, TREE>(a);
}

template <bool TREE>
void launch_pool(const VerifyLaunch& a, int page_size, int nw) {
    switch (page_size) {
        case 8: launch_page<8, TREE>(a, nw); break;
        case 16: launch_page<16, TREE>(a, nw); break;
        case 32: launch_page<32, TREE>(a, nw); break;
        default: launch_page<64, TREE>(a, nw); break;
    }
}

// Row tables of a verify pass.  One workgroup per sequence, one thread per
// row: row 0 of sequence b is its pending id next[b], rows 1..len-1 its drafts
// (packed in sequence order, b's from drafts[doff[b]]); tgt[row] is the id the row
// has to predict for the next draft to be accepted (the next row's token, -1
// for the last row).
__global__ __launch_bounds__(64) void verify_rows_kernel(const int* __restrict__ next, const int* __restrict__ drafts,
                                                         const int* __restrict__ doffs,
                                                         const int* __restrict__ start, const int* __restrict__ row0,
                                                         const int* __restrict__ len, int* __restrict__ tok,
                                                         int* __restrict__ pos, int* __restrict__ seq,
                                                         int* __restrict__ tgt) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = len[b];
    if (t >= n) return;
    const int r = row0[b] + t;
    const int doff = doffs[b];
    tok[r] = t == 0 ? next[b] : drafts[doff + t - 1];
    pos[r] = start[b] + t;
    seq[r] = b;
    tgt[r] = t + 1 < n ? drafts[doff + t] : -1;
}

// The accept decision, one thread per sequence: a = the number of leading
// drafts that equal the greedy id of the row before them.
__global__ __launch_bounds__(64) void verify_accept_kernel(const int* __restrict__ tok, const int* __restrict__ top,
                                                           const int* __restrict__ start,
                                                           const int* __restrict__ row0, const int* __restrict__ len,
                                                           int B, int* __restrict__ n_accepted,
                                                           int* __restrict__ cont_row, int* __restrict__ pos) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int n = len[b];
    if (n <= 0) {  // untouched: position left as it is
        n_accepted[b] = -1;
        cont_row[b] = -1;
        return;
    }
    const int r0 = row0[b];
    int a = 0;
    while (a + 1 < n && tok[r0 + a + 1] == top[r0 + a]) ++a;
    n_accepted[b] = a;
    cont_row[b] = r0 + a;
    pos[b] = start[b] + a;
}

// Row tables of a tree pass, the sibling of verify_rows_kernel: node 0 of
// sequence b is its pending id, node j + 1 its draft j with parent node
// parents[doff + j] in [0, j] (a smaller index than the child's: node order is
// topological).  Per row: the token, pos = start + depth (what the embedding
// reads), slot = start + node index (where the row's K/V is appended) and the
// ancestor mask (bit i: node i is the node itself or one of its ancestors).
// A parent outside [0, j] is clamped into it, so the walk ends within t steps
// whatever the table holds (the engine refuses such a table on the host).
__global__ __launch_bounds__(64) void verify_tree_rows_kernel(
    const int* __restrict__ next, const int* __restrict__ drafts, const int* __restrict__ parents,
    const int* __restrict__ doffs, const int* __restrict__ start, const int* __restrict__ row0,
    const int* __restrict__ len, int* __restrict__ tok, int* __restrict__ pos, int* __restrict__ seq,
    int* __restrict__ slot, unsigned char* __restrict__ anc) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = min(len[b], HPA_VERIFY_MAX_ROWS);
    if (t >= n) return;
    const int r = row0[b] + t;
    const int doff = doffs[b];
    unsigned mask = 1u;
    int depth = 0;
    for (int cur = t; cur > 0; ++depth) {
        mask |= 1u << cur;
        cur = min(max(parents[doff + cur - 1], 0), cur - 1);
    }
    tok[r] = t == 0 ? next[b] : drafts[doff + t - 1];
    pos[r] = start[b] + depth;
    slot[r] = start[b] + t;
    seq[r] = b;
    anc[r] = (unsigned char)mask;
}

// The accept walk, one thread per sequence: from the root, step to the
// lowest-indexed child whose token is the greedy id of the node it hangs from,
// for as long as there is one.  path [B][HPA_VERIFY_MAX_ROWS]: the node indices
// of the accepted drafts, strictly increasing.
__global__ __launch_bounds__(64) void verify_tree_accept_kernel(
    const int* __restrict__ tok, const int* __restrict__ top, const int* __restrict__ parents,
    const int* __restrict__ doffs, const int* __restrict__ start, const int* __restrict__ row0,
    const int* __restrict__ len, int B, int* __restrict__ n_accepted, int* __restrict__ path,
    int* __restrict__ cont_row, int* __restrict__ pos) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int n = min(len[b], HPA_VERIFY_MAX_ROWS);
    if (n <= 0) {  // untouched: position left as it is
        n_accepted[b] = -1;
        cont_row[b] = -1;
        return;
    }
    const int r0 = row0[b], doff = doffs[b];
    int cur = 0, a = 0;
    for (;;) {
        const int want = top[r0 + cur];
        int c = cur + 1;
        while (c < n && !(parents[doff + c - 1] == cur && tok[r0 + c] == want)) ++c;
        if (c >= n) break;
        path[b * HPA_VERIFY_MAX_ROWS + a++] = c;  // c > cur: at most n - 1 steps
        cur = c;
    }
    n_accepted[b] = a;
    cont_row[b] = r0 + cur;
    pos[b] = start[b] + a;
}

// K/V compaction after a tree pass (hpa_pool_compact_path): grid (sequence,
// layer).  A thread owns fixed 16-byte lanes -- (K|V, head, 4 dims) -- of the
// slot rows and moves, for k = 1 .. a in ascending order, its lane of slot
// start + path[k-1] to slot start + k.  In place and safe: path strictly
// increases and path[k-1] >= k, so the destination k lies below every source
// still to be read (path[k'-1] >= k' > k for k' > k), and each lane is read
// and written by one thread only.  Pages come from the block table: source
// and destination may lie in different pages.  An entry that breaks the
// invariant, or a slot without a page, is skipped.
constexpr int kCompactThreads = 256;
__global__ __launch_bounds__(kCompactThreads) void pool_compact_path_kernel(
    float* __restrict__ base, size_t layer_elems, size_t page_elems, int NH, int P,
    const int* __restrict__ block_table, int bt_stride, const int* __restrict__ start,
    const int* __restrict__ path, const int* __restrict__ n_accepted) {
    const int b = blockIdx.x;
    const int a = min(n_accepted[b], HPA_VERIFY_MAX_ROWS - 1);
    if (a <= 0) return;
    const int st = start[b];
    float* layer = base + (size_t)blockIdx.y * layer_elems;
    const int* bt = block_table + (size_t)b * bt_stride;
    const int lanes = 2 * NH * 16;
    for (int k = 1; k <= a; ++k) {
        const int src = path[b * HPA_VERIFY_MAX_ROWS + k - 1];
        if (src <= k || src >= HPA_VERIFY_MAX_ROWS) continue;  // in place already (== k), or not a path
        const int ss = st + src, ds = st + k;
        if (ss / P >= bt_stride) continue;
        const int sp = bt[ss / P], dp = bt[ds / P];
        if (sp < 0 || dp < 0) continue;
        for (int i = threadIdx.x; i < lanes; i += kCompactThreads) {
            const int kv = i / (NH * 16), head = (i >> 4) % NH, d = (i & 15) * 4;
            const size_t so = hpa::kv_tile_off(sp, page_elems, NH, kv, head, P) +
                              (kv == 0 ? hpa::kv_k_chunk<4>(d, ss % P, P) : hpa::kv_v_off(d, ss % P));
            const size_t dof = hpa::kv_tile_off(dp, page_elems, NH, kv, head, P) +
                               (kv == 0 ? hpa::kv_k_chunk<4>(d, ds % P, P) : hpa::kv_v_off(d, ds % P));
            *reinterpret_cast<float4*>(layer + dof) = *reinterpret_cast<const float4*>(layer + so);
        }
    }
}

}  // namespace

extern "C" {

int hpa_paged_attention_verify(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                               int bt_stride, const int* start, const int* row0, const int* len, int B, int T,
                               float* out_frag) {
    HPA_REQUIRE(pool && pool->base && pool->head_size == HS, "verify attention: pool with head_size 64");
    HPA_REQUIRE(pool->dtype == HPA_F32, "verify attention: fp32 pool (bf16 and fp8 pools: the prefill kernel)");
    HPA_REQUIRE(pool->page_size == 8 || pool->page_size == 16 || pool->page_size == 32 || pool->page_size == 64,
                "verify attention: page size must be 8, 16, 32 or 64");
    HPA_REQUIRE(layer >= 0 && layer < pool->num_layers, "verify attention: layer out of range");
    HPA_REQUIRE(q && block_table && start && out_frag && B > 0 && bt_stride > 0, "verify attention: bad arguments");
    HPA_REQUIRE(T >= 1 && T <= HPA_VERIFY_MAX_ROWS, "verify attention: 1..HPA_VERIFY_MAX_ROWS rows per sequence");
    HPA_REQUIRE(!row0 == !len, "verify attention: row0 and len go together");
    HPA_REQUIRE(((uintptr_t)out_frag & 15) == 0, "verify attention: out must be 16-byte aligned");
    VerifyLaunch a;
    a.q = q;
    a.base = (const float*)pool->base + (size_t)layer * pool->layer_elems;
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
    // 4 or 8 waves: the process-wide override (timing tools, tests) where it names one of them, else by shape
    const int forced = hpa_attention_waves();
    const int nw = forced == 4 || forced == 8 ? forced : hpa_attn_pick_waves(B, pool->num_heads, 1, hpa::num_cus());
    a.anc = nullptr;
    launch_pool<false>(a, pool->page_size, nw);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_paged_attention_verify_tree(const float* q, const HpaKVPool* pool, int layer, const int* block_table,
                                    int bt_stride, const int* start, const int* row0, const int* len,
                                    const unsigned char* anc, int B, int T, float* out_frag) {
    HPA_REQUIRE(pool && pool->base && pool->head_size == HS, "tree attention: pool with head_size 64");
    HPA_REQUIRE(pool->dtype == HPA_F32, "tree attention: fp32 pool (the prefill kernel has no tree mask)");
    HPA_REQUIRE(pool->page_size == 8 || pool->page_size == 16 || pool->page_size == 32 || pool->page_size == 64,
                "tree attention: page size must be 8, 16, 32 or 64");
    HPA_REQUIRE(layer >= 0 && layer < pool->num_layers, "tree attention: layer out of range");
    HPA_REQUIRE(q && block_table && start && out_frag && anc && B > 0 && bt_stride > 0, "tree attention: bad arguments");
    HPA_REQUIRE(T >= 1 && T <= HPA_VERIFY_MAX_ROWS, "tree attention: 1..HPA_VERIFY_MAX_ROWS nodes per sequence");
    HPA_REQUIRE(!row0 == !len, "tree attention: row0 and len go together");
    HPA_REQUIRE(((uintptr_t)out_frag & 15) == 0, "tree attention: out must be 16-byte aligned");
    VerifyLaunch a;
    a.q = q;
    a.base = (const float*)pool->base + (size_t)layer * pool->layer_elems;
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
    const int forced = hpa_attention_waves();  // as hpa_paged_attention_verify
    const int nw = forced == 4 || forced == 8 ? forced : hpa_attn_pick_waves(B, pool->num_heads, 1, hpa::num_cus());
    launch_pool<true>(a, pool->page_size, nw);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_verify_tree_rows(const int* next, const int* drafts, const int* parents, const int* draft0, const int* start,
                         const int* row0, const int* len, int B, int* tok, int* pos, int* seq, int* slot,
                         unsigned char* anc) {
    HPA_REQUIRE(next && drafts && parents && draft0 && start && row0 && len && tok && pos && seq && slot && anc && B > 0,
                "verify tree rows: bad arguments");
    verify_tree_rows_kernel<<<(unsigned)B, 64, 0, hpa_stream()>>>(next, drafts, parents, draft0, start, row0, len, tok,
                                                                 pos, seq, slot, anc);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_verify_tree_accept(const int* tok, const int* top_id, const int* parents, const int* draft0, const int* start,
                           const int* row0, const int* len, int B, int* n_accepted, int* path, int* cont_row,
                           int* pos) {
    HPA_REQUIRE(tok && top_id && parents && draft0 && start && row0 && len && n_accepted && path && cont_row && pos &&
                    B > 0,
                "verify tree accept: bad arguments");
    verify_tree_accept_kernel<<<(unsigned)((B + 63) / 64), 64, 0, hpa_stream()>>>(
        tok, top_id, parents, draft0, start, row0, len, B, n_accepted, path, cont_row, pos);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_pool_compact_path(const HpaKVPool* pool, const int* block_table, int bt_stride, const int* start,
                          const int* path, const int* n_accepted, int B) {
    HPA_REQUIRE(pool && pool->base && block_table && start && path && n_accepted && B > 0 && bt_stride > 0,
                "compact_path: bad arguments");
    HPA_REQUIRE(pool->dtype == HPA_F32 && pool->head_size == HS, "compact_path: fp32 pool with head_size 64");
    HPA_REQUIRE(pool->num_layers <= 65535, "compact_path: too many layers");
    const dim3 grid((unsigned)B, (unsigned)pool->num_layers);
    pool_compact_path_kernel<<<grid, kCompactThreads, 0, hpa_stream()>>>(
        (float*)pool->base, pool->layer_elems, pool->page_elems, pool->num_heads, pool->page_size, block_table,
        bt_stride, start, path, n_accepted);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_verify_rows(const int* next, const int* drafts, const int* draft0, const int* start, const int* row0,
                    const int* len, int B, int* tok, int* pos, int* seq, int* target) {
    HPA_REQUIRE(next && drafts && draft0 && start && row0 && len && tok && pos && seq && target && B > 0,
                "verify rows: bad arguments");
    verify_rows_kernel<<<(unsigned)B, 64, 0, hpa_stream()>>>(next, drafts, draft0, start, row0, len, tok, pos, seq,
                                                            target);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_verify_accept(const int* tok, const int* top_id, const int* start, const int* row0, const int* len, int B,
                      int* n_accepted, int* cont_row, int* pos) {
    HPA_REQUIRE(tok && top_id && start && row0 && len && n_accepted && cont_row && pos && B > 0,
                "verify accept: bad arguments");
    verify_accept_kernel<<<(unsigned)((B + 63) / 64), 64, 0, hpa_stream()>>>(tok, top_id, start, row0, len, B,
                                                                            n_accepted, cont_row, pos);
    HPA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
