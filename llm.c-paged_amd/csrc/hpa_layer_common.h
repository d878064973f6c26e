// hpa_layer_common.h -- what the decode layer's translation units share:
// hpa_layer.hip (the extern "C" surface), hpa_layer_units.hip (forms 0..5),
// hpa_chain6.hip (form 6 and the step's first launch), hpa_chain8.hip (form 8).
// The kernel arguments of every form, the trace macros, the LayerNorm fold,
// the counter layout and the epilogue folds of the two 12-wave chains, and
// the launch functions hpa_decode_layer calls.  Internal: no public header
// declares any of it.
#pragma once
#include <math.h>
#include <string.h>

#include "hpa_attn_body.h"
#include "hpa_gemm_body.h"
#include "hpa_handoff.h"

namespace {
using hpa_attn::HS;
using hpa_attn::kRec;
using hpa::drain_vm;
using hpa::kPad;
using hpa::ld4;
using hpa::lds_barrier;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// forms 0..5: counters ATT, X1, H, X2 x 8 shards
constexpr int kCtrInts = 4 * 8 * kPad;

template <int NH>
struct LD {
    static constexpr int C = 64 * NH;
    static constexpr int K16 = C / 16;  // k16 steps of K = C; also the column tiles of N = C
    static constexpr int NCT = C / 16;
    static constexpr int FP = 4;   // fcproj K parts (C each)
    static constexpr int SW = NH;  // k16 steps per wave: K = C over a slot's 4 waves
};

struct KA {
    int B, Mp, R, S, G, last, layer;
    const float* q;
    const void* kv;       // layer l of the pool
    void* kv_next;        // layer l+1
    size_t page_elems;
    const int* bt;
    int bt_stride;
    const int* pos;
    float qscale, m_init;
    float *att, *res, *res2, *fch;
    const float *w_ap, *b_ap, *w_fc, *fc_c1, *fc_c2, *w_fp, *b_fp, *w_qkv, *qkv_c1, *qkv_c2;
    float* q_out;
    float* stats_out;
    float* rec;
    float* slab_fp;
    int* ctr;
    int* err;
    int* err_sticky;
    // chain form 8 (wide layers, GPT-2 XL): tiles per unit and tile groups
    // (padded to a multiple of 8) of attproj, fc, fcproj, qkv
    int xt[4], xng[4];
    // the step's first launch (decode_first6_kernel): the tokens, the
    // embedding tables, and the step's counter block to zero (16-B granules)
    const int* tokens;
    const float *wte, *wpe;
    int4* zero;
    int zero_n4;
    // fp8 pool (chain form 6 and the first launch only): the (scale, inv)
    // pairs [2][NH][2] of the layer at kv_next, device memory read at run time;
    // NULL: an fp32 / bf16 pool
    const float* kv_scales_next;
};

// diagnostic build (-DHPA_LAYER_TRACE, tools/pl_trace.py): s_memrealtime of
// workgroup-level events per (layer, workgroup); never in the product library.
// Each kernel file defines its own g_pl_trace[64][256][16] (hpa_chain8.hip
// also g_cx_wave[256][12][16]) before its kernels.
#ifdef HPA_LAYER_TRACE
// (the stamp intrinsic counts as a memory clobber: the trace build loads q
// through vector loads + readfirstlane, HPA_PL_QREG, ~1 us later than the
// product's scalar loads)
#ifndef HPA_PL_QREG
#define HPA_PL_QREG 1
#endif
#define CX_WSTAMP(on, slot)                                                                              \
    do {                                                                                                 \
        if ((on) && (threadIdx.x & 63) == 0 && blockIdx.x < 256)                                         \
            g_cx_wave[blockIdx.x][threadIdx.x >> 6][slot] = (unsigned long long)__builtin_amdgcn_s_memtime(); \
    } while (0)
#define PL_MARK(k)                                                                                     \
    do {                                                                                               \
        if (threadIdx.x == 0 && a.layer < 64 && blockIdx.x < 256)                                      \
            g_pl_trace[a.layer][blockIdx.x][k] = (unsigned long long)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
// stamps taken before the attention are stored after it: a global store in
// front of the q loads would cost them their scalar (s_load) form
#define PL_STAMP(var) const unsigned long long var = (unsigned long long)__builtin_amdgcn_s_memrealtime()
#define PL_STORE(k, var)                                                           \
    do {                                                                           \
        if (threadIdx.x == 0 && a.layer < 64 && blockIdx.x < 256) g_pl_trace[a.layer][blockIdx.x][k] = var; \
    } while (0)
#else
#define PL_MARK(k) \
    do {           \
    } while (0)
#define PL_STAMP(var) \
    do {              \
    } while (0)
#define PL_STORE(k, var) \
    do {                 \
    } while (0)
#define CX_WSTAMP(on, slot) \
    do {                    \
    } while (0)
#endif

__device__ __forceinline__ float4 ld_nt(const float4* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// LayerNorm-folded value: rstd*(acc - mean*c1) + c2 (Epi::apply's order);
// the row partial sums of the NWU waves of unit slot us
template <int NWU = 4>
__device__ __forceinline__ float ln_fold_val(const float* wsum, int us, int lrow, int K, float val, float c1,
                                             float c2) {
    const float* ws = wsum + us * NWU * 32;
    float S1 = ws[2 * lrow], S2 = ws[2 * lrow + 1];
#pragma unroll
    for (int ww = 1; ww < NWU; ++ww) {
        S1 += ws[ww * 32 + 2 * lrow];
        S2 += ws[ww * 32 + 2 * lrow + 1];
    }
    const float m = S1 / K;
    const float rstd = 1.0f / sqrtf(fmaxf(S2 / K - m * m, 0.f) + 1e-5f);
    val = rstd * (val - m * c1);
    val += c2;
    return val;
}

// ------------------------------------------------------------------ the 12-wave chains (forms 6 and 8)
// one unit of all 12 waves per workgroup; what the two forms share: the
// counter layout (hpa_decode_layer_sizes), the sharded wait and arrive, and
// the 16-byte epilogue folds
namespace chain {
constexpr int NW = 12;  // waves per workgroup = waves per unit
// wait counters: X1 per row block, H per (row block, K part), X2 per row block
enum { X1 = 0, H = 4, X2 = 20, NCTR = 24 };
constexpr int kCtr = NCTR * 8 * kPad;  // ints of the sharded counters; the fcproj tickets follow
// form 6 (HPA_C6_GW): 16-column tiles landed per (row block, 64-column k-group) of each
// phase's A, after the tickets: res2 for fc (12 groups per row block), fch for
// fcproj (48), res for qkv (12); one 128-B line each
constexpr int kGC = 0, kGD = 4 * NW * kPad, kGE = kGD + 4 * 4 * NW * kPad;
constexpr int kGrp = kGE + 4 * NW * kPad;

__device__ __forceinline__ void arrive6(const KA& a, int ctr, int n) { hpa::arrive_shard(a.ctr + ctr * 8 * kPad, n); }

// every thread calls; until the 8 shards of counter ctr sum to `expected` (hpa::wait_wg)
template <typename SM>
__device__ __forceinline__ bool wait6(const KA& a, int ctr, int expected, int code, SM& sm) {
    return hpa::wait_wg(a.err, a.err_sticky, code, sm.s_ok,
                        [&] { return hpa::shards_reached(a.ctr + ctr * 8 * kPad, expected); });
}

__device__ __forceinline__ void publish6(const KA& a, int ctr, bool did) {
    drain_vm();
    lds_barrier();
    if (threadIdx.x == 0 && did) arrive6(a, ctr, 1);
}

// epilogue thread tid < T*64: tile t = tid / 64, row r = (tid % 64) / 4,
// columns 4q .. 4q+3 (q = tid % 4) of that tile; its 4 values summed over the
// 12 waves in wave order.  red is [wave][TS tiles][256]
template <int TS>
__device__ __forceinline__ float4 fold_t(const float* red, int t, int r, int q) {
    const float* p = red + t * 256 + (r & 3) * 64 + 16 * (r >> 2) + 4 * q;
    float4 v = *reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        const float4 x = *reinterpret_cast<const float4*>(p + w * TS * 256);
        v.x += x.x;
        v.y += x.y;
        v.z += x.z;
        v.w += x.w;
    }
    return v;
}

// LN fold of 4 values of row r over K columns (ln_fold_val<12>, elementwise)
__device__ __forceinline__ float4 ln_fold4(const float* wsum, int r, int K, float4 v, float4 c1, float4 c2) {
    v.x = ln_fold_val<NW>(wsum, 0, r, K, v.x, c1.x, c2.x);
    v.y = ln_fold_val<NW>(wsum, 0, r, K, v.y, c1.y, c2.y);
    v.z = ln_fold_val<NW>(wsum, 0, r, K, v.z, c1.z, c2.z);
    v.w = ln_fold_val<NW>(wsum, 0, r, K, v.w, c1.w, c2.w);
    return v;
}
}  // namespace chain

// kernel arguments of one layer launch (every form; KA is private to each
// translation unit, so this is too: emitted where a launcher uses it)
inline void fill_ka(const HpaLayerArgs* h, int G, KA& a) {
    const HpaKVPool* pool = h->pool;
    a.B = h->B;
    a.R = (h->B + 15) / 16;
    a.Mp = h->stats_mp > 0 ? h->stats_mp : a.R * 16;  // the stride of stats_out only
    a.S = h->splits;
    a.G = G;
    a.last = h->last;
    a.layer = h->layer;
    a.q = h->q;
    a.kv = (const char*)pool->base + (size_t)h->layer * pool->layer_elems * pool->elem_bytes;
    a.kv_next = h->last ? nullptr : (char*)pool->base + (size_t)(h->layer + 1) * pool->layer_elems * pool->elem_bytes;
    a.page_elems = pool->page_elems;
    a.bt = h->block_table;
    a.bt_stride = h->bt_stride;
    a.pos = h->pos;
    const float log2e = 1.4426950408889634f;
    a.qscale = (float)(1.0 / sqrt((double)HS)) * log2e;
    a.m_init = -10000.0f * log2e;
    a.att = h->att;
    a.res = h->res;
    a.res2 = h->res2;
    a.fch = h->fch;
    a.w_ap = h->w_ap;
    a.b_ap = h->b_ap;
    a.w_fc = h->w_fc;
    a.fc_c1 = h->fc_c1;
    a.fc_c2 = h->fc_c2;
    a.w_fp = h->w_fp;
    a.b_fp = h->b_fp;
    a.w_qkv = h->w_qkv;
    a.qkv_c1 = h->qkv_c1;
    a.qkv_c2 = h->qkv_c2;
    a.q_out = h->q_out;
    a.stats_out = h->stats_out;
    a.rec = h->rec;
    a.slab_fp = h->slab;
    a.ctr = h->counters;
    a.err = h->err;
    a.err_sticky = h->err_sticky;
    a.kv_scales_next = pool->dtype == HPA_FP8 && !h->last
                           ? pool->scales + (size_t)(h->layer + 1) * 4 * pool->num_heads
                           : nullptr;
}

}  // namespace

// what hpa_layer.hip calls (G: the CU count = the grid)
int hpa_layer_units_launch(const HpaLayerArgs* h, int G);  // forms 0..5 (hpa_layer_units.hip)
int hpa_chain6_launch(const HpaLayerArgs* h, int G);       // form 6 (hpa_chain6.hip)
int hpa_chain8_launch(const HpaLayerArgs* h, int G);       // form 8 (hpa_chain8.hip)
// form 8's tiles per unit and tile groups of its four phases; nonzero: no shape
int hpa_chain8_shape(int B, int NH, int G, int xt[4], int xng[4]);
#ifdef HPA_LAYER_TRACE
// one file's stamp array `sym` ([64][256][16] u64; a __device__ array is private
// to its translation unit): host NULL clears it, else its first `layers` layers
// are ADDED to host (one form runs in a traced step: the other arrays are 0)
int hpa_pl_trace_add(const void* sym, unsigned long long* host, int layers);  // hpa_layer.hip
int hpa_layer_units_trace(unsigned long long* host, int layers);  // hpa_pl_trace_add on the file's own stamps
int hpa_chain6_trace(unsigned long long* host, int layers);
int hpa_chain8_trace(unsigned long long* host, int layers);
#endif
