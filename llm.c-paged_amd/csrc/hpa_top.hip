// hpa_top.hip -- the k most likely columns of every logits row with their
// log-probabilities (top_logprobs), the row's log-sum-exp and one target
// column's log-probability.
//
// Order.  Entry j of a row is its j-th element under: logit descending as a
// float comparison (-0.0 and +0.0 tie), equal logits by ascending column.
// Columns are distinct, so this is a total order and the answer does not
// depend on the launch shape.
//
// Two launches:
//   top_slice_kernel  the row is cut as in hpa_logits_process (peeled head,
//                     aligned float4s, peeled tail; slice 0 takes the head, the
//                     last slice the tail), one slice per WAVE, four waves to
//                     a workgroup on a (slice / 4, row) grid.  A slice is at
//                     most 256 float4s, so a wave reads its part ONCE into
//                     registers (four 16-byte loads per lane and two scalars),
//                     leaves (max, sum exp(x - max)) and runs k rounds of a
//                     wave arg-max with removal: every lane keeps the best of
//                     its own registers; a round is two DPP reductions (the
//                     largest value, then the lowest column among the lanes
//                     that hold it) and only the winning lane rescans its
//                     registers.  No LDS and no barrier.  A slice with fewer
//                     than k columns pads with (-inf, INT_MAX).
//   top_final_kernel  one workgroup per row: the S sorted candidate lists go
//                     to LDS and lane s walks list s; k rounds of the same
//                     arg-max over the lists' heads are the S-way merge.  One
//                     wave (no barrier in a round) up to 64 slices, which is
//                     every shape up to V = 65536; four waves and one barrier
//                     per round above.
// A removed or absent register holds -inf, which no finite logit ties with.
// (profiles/EXPERIMENTS.md "Top log-probabilities": the rounds are bound by
// their dependent latency, so a round over a workgroup -- butterfly shuffles,
// an LDS exchange and a barrier -- took three times as long.)
//
// Log-sum-exp and its error against the float64 log-softmax of the same fp32
// logits.  Slice s: m_s = max, S_s = sum expf(x - m_s) in double, every lane its
// registers in a fixed order, lanes by a wave butterfly (a + b == b + a, so
// every lane holds the same bits).  Row: M = max m_s, S = sum_s S_s exp(m_s - M)
// in double (lane s its term, the same butterfly, then the waves in order),
// lse = M + log S.  Terms: expf is good to 2 ulp (2.4e-7 relative); its
// argument x - m_s is rounded once in fp32, |d| 2^-24 on a term e^d, which
// relative to S is sum |d_i| e^d_i / sum e^d_i * 2^-24 <= ln(V) 2^-24 (a term far
// below the maximum weighs nothing unless e^|d| of them exist): 6.4e-7 at
// V = 50257.  The double additions, the double exp of the rescale and log add
// nothing visible.  So |lse - lse64| < 9e-7, and a log-probability
// (float)((double)x - lse) adds one rounding, 2^-24 max(|lse|, |x|): inside the
// project's 4e-6 + 2^-22 max(|lse|, |x|) (tests/score_ref64.py).
// No floating-point atomics and no order that depends on scheduling: a launch
// repeats bit for bit.
#include <limits.h>
#include <math.h>

#include "hpa_internal.h"

namespace {
constexpr int kTsThreads = 256;
constexpr int kTsWaves = kTsThreads / 64;          // slices per workgroup of the slice kernel
constexpr int kTsLoads = 4;                        // 16-byte loads per lane: the whole slice in registers
constexpr int kTsSliceQ = 64 * kTsLoads;           // float4s per slice at most
constexpr int kTsSlots = 4 * kTsLoads + 2;         // a lane's values: head scalar, loads, tail scalar
constexpr int kTsMaxSlices = 256;                  // one lane of the final workgroup per slice
constexpr int kTsOneWave = 64;                     // slices the final kernel merges in one wave

// wave64 reductions on DPP (row_shr 1/2/4/8, row_bcast 15/31 as hpa_fused.hip's
// scan: VALU lane moves, no LDS round trips); lane 63 holds the result and a
// scalar read hands it to every lane
template <int CTRL, int ROWS>
__device__ __forceinline__ int top_dpp(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWS, 0xf, false);
}
__device__ __forceinline__ float wave_max_all(float v) {
    const int none = __float_as_int(-INFINITY);
    v = fmaxf(v, __int_as_float(top_dpp<0x111, 0xf>(none, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(top_dpp<0x112, 0xf>(none, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(top_dpp<0x114, 0xf>(none, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(top_dpp<0x118, 0xf>(none, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(top_dpp<0x142, 0xa>(none, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(top_dpp<0x143, 0xc>(none, __float_as_int(v))));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_min_all(int v) {
    v = min(v, top_dpp<0x111, 0xf>(INT_MAX, v));
    v = min(v, top_dpp<0x112, 0xf>(INT_MAX, v));
    v = min(v, top_dpp<0x114, 0xf>(INT_MAX, v));
    v = min(v, top_dpp<0x118, 0xf>(INT_MAX, v));
    v = min(v, top_dpp<0x142, 0xa>(INT_MAX, v));
    v = min(v, top_dpp<0x143, 0xc>(INT_MAX, v));
    return __builtin_amdgcn_readlane(v, 63);
}
// the wave's best (value, column) of every lane's (bv, bi): the largest value,
// then the lowest column among the lanes that hold it (INT_MAX: none left)
__device__ __forceinline__ void wave_top(float bv, int bi, float& wv, int& wi) {
    wv = wave_max_all(bv);
    wi = wave_min_all(bv == wv ? bi : INT_MAX);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}

// (v, i) beats (bv, bi): the larger value, then the lower column
__device__ __forceinline__ void top_take(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

// the workspace of `rows` rows cut into S slices: sum [rows][S] double,
// max [rows][S] float, candidate values and columns [rows][S][k]
struct TopWs {
    double* sum;
    float* mx;
    float* cv;
    int* ci;
};
inline size_t top_ws_bytes(size_t cells, size_t k) { return cells * (12 + 8 * k); }
inline TopWs top_ws_cut(void* ws, size_t cells, size_t k) {
    TopWs w;
    w.sum = (double*)ws;
    w.mx = (float*)(w.sum + cells);
    w.cv = w.mx + cells;
    w.ci = (int*)(w.cv + cells * k);
    return w;
}

__global__ __launch_bounds__(kTsThreads) void top_slice_kernel(const float* __restrict__ logits, int V, int k, int S,
                                                              const int* __restrict__ active,
                                                              double* __restrict__ ws_sum, float* __restrict__ ws_mx,
                                                              float* __restrict__ ws_cv, int* __restrict__ ws_ci) {
    const int b = blockIdx.y, t = threadIdx.x & 63;
    const int s = blockIdx.x * kTsWaves + (threadIdx.x >> 6);  // this wave's slice
    if (s >= S || (active && active[b] <= 0)) return;          // wave-uniform; an inactive row is left as it is
    const float* lg = logits + (size_t)b * V;
    // head scalars, nq aligned float4s from lg + head, tail scalars from tail0
    const int head = min(V, (int)((4u - (unsigned)(((size_t)lg >> 2) & 3u)) & 3u));
    const int nq = (V - head) >> 2, tail0 = head + 4 * nq;
    const int Q = (nq + S - 1) / S;  // <= kTsSliceQ (the launcher's slice count)
    const int qlo = min(nq, s * Q), qhi = min(nq, qlo + Q);

    // x[0] the head scalar (column t), x[1 + 4u + j] component j of load u, x[last] the tail scalar
    float x[kTsSlots];
#pragma unroll
    for (int i = 0; i < kTsSlots; ++i) x[i] = -INFINITY;
    if (s == 0 && t < head) x[0] = lg[t];
    const float4* lq = reinterpret_cast<const float4*>(lg + head);
#pragma unroll
    for (int u = 0; u < kTsLoads; ++u) {
        const int q = qlo + t + u * 64;
        if (q < qhi) {
            const float4 v = lq[q];
            x[1 + 4 * u] = v.x;
            x[2 + 4 * u] = v.y;
            x[3 + 4 * u] = v.z;
            x[4 + 4 * u] = v.w;
        }
    }
    if (s == S - 1 && t < V - tail0) x[kTsSlots - 1] = lg[tail0 + t];
    // the lane's best (bv in slot bs, column bi): a slot's column increases with the slot, so the
    // strict > keeps the lowest column of equals
    float bv;
    int bi, bs;
    auto rescan = [&]() {
        bv = -INFINITY;
        bs = -1;
#pragma unroll
        for (int i = 0; i < kTsSlots; ++i)
            if (x[i] > bv) {
                bv = x[i];
                bs = i;
            }
        bi = bs < 0 ? INT_MAX
             : bs == 0 ? t
             : bs == kTsSlots - 1 ? tail0 + t
                                  : head + 4 * (qlo + t + ((bs - 1) >> 2) * 64) + ((bs - 1) & 3);
    };
    rescan();

    // (max, sum exp) of the slice
    const float m = wave_max_all(bv);
    double sum = 0.0;
    if (m != -INFINITY) {  // an empty slice sums nothing
#pragma unroll
        for (int i = 0; i < kTsSlots; ++i) sum += (double)expf(x[i] - m);  // absent: exp(-inf) = 0
    }
    sum = wave_sum_f64(sum);
    const size_t cell = (size_t)b * S + s;
    if (t == 0) {
        ws_sum[cell] = sum;
        ws_mx[cell] = m;
    }

    // k rounds of arg-max with removal
    for (int j = 0; j < k; ++j) {
        float wv;
        int wi;
        wave_top(bv, bi, wv, wi);
        if (wi == INT_MAX) {  // fewer than k columns in the slice: padding that no merge takes
            if (t == 0) {
                ws_cv[cell * k + j] = -INFINITY;
                ws_ci[cell * k + j] = INT_MAX;
            }
        } else if (bi == wi) {  // the winning lane: its own value (the sign of a zero is the column's)
            ws_cv[cell * k + j] = bv;
            ws_ci[cell * k + j] = bi;
#pragma unroll
            for (int i = 0; i < kTsSlots; ++i)
                if (i == bs) x[i] = -INFINITY;
            rescan();
        }
    }
}

struct TfShared {
    float red_m[kTsWaves];
    double red_s[kTsWaves];
    float rv[2][kTsWaves];  // by round parity: one barrier per round
    int ri[2][kTsWaves];
};

// blockDim.x = 64 (S <= 64) or 256; dynamic LDS: S * k values, then S * k columns
__global__ __launch_bounds__(kTsThreads) void top_final_kernel(const float* __restrict__ logits, int V, int k, int S,
                                                              const int* __restrict__ active,
                                                              const int* __restrict__ targets,
                                                              const double* __restrict__ ws_sum,
                                                              const float* __restrict__ ws_mx,
                                                              const float* __restrict__ ws_cv,
                                                              const int* __restrict__ ws_ci, int* __restrict__ top_ids,
                                                              float* __restrict__ top_lps, float* __restrict__ target_lp,
                                                              float* __restrict__ lse_out) {
    extern __shared__ float dyn[];
    __shared__ TfShared sh;
    const int b = blockIdx.x, t = threadIdx.x, nw = blockDim.x >> 6;
    if (active && active[b] <= 0) return;  // row left as it is
    float* cv = dyn;
    int* ci = reinterpret_cast<int*>(dyn + (size_t)S * k);
    const size_t row0 = (size_t)b * S;
    for (int i = t; i < S * k; i += blockDim.x) {
        cv[i] = ws_cv[row0 * k + i];
        ci[i] = ws_ci[row0 * k + i];
    }

    // lse = M + log(sum_s S_s exp(m_s - M)): lane s its slice, fixed tree
    const float ms = t < S ? ws_mx[row0 + t] : -INFINITY;
    float M = wave_max_all(ms);
    if (nw > 1) {
        if ((t & 63) == 0) sh.red_m[t >> 6] = M;
        __syncthreads();
        for (int w = 0; w < nw; ++w) M = fmaxf(M, sh.red_m[w]);
    }
    double term = 0.0;
    if (t < S && ms != -INFINITY) term = ws_sum[row0 + t] * exp((double)ms - (double)M);
    term = wave_sum_f64(term);
    if (nw > 1) {
        if ((t & 63) == 0) sh.red_s[t >> 6] = term;
        __syncthreads();
        term = sh.red_s[0];
        for (int w = 1; w < nw; ++w) term += sh.red_s[w];
    }
    const double lse = (double)M + log(term);
    if (t == 0) {
        if (lse_out) lse_out[b] = (float)lse;
        if (target_lp) {
            const int tg = targets ? targets[b] : -1;
            target_lp[b] = tg < 0 || tg >= V ? 0.0f : (float)((double)logits[(size_t)b * V + tg] - lse);
        }
    }
    __syncthreads();  // the candidate lists are in LDS

    // S-way merge: lane s holds the head of list s
    int p = 0;
    float hv = t < S ? cv[t * k] : -INFINITY;
    int hi = t < S ? ci[t * k] : INT_MAX;
    for (int j = 0; j < k; ++j) {
        float wv;
        int wi;
        wave_top(hv, hi, wv, wi);
        if (nw > 1) {
            const int par = j & 1;
            if ((t & 63) == 0) {
                sh.rv[par][t >> 6] = wv;
                sh.ri[par][t >> 6] = wi;
            }
            __syncthreads();
            wv = sh.rv[par][0];
            wi = sh.ri[par][0];
            for (int w = 1; w < nw; ++w) top_take(wv, wi, sh.rv[par][w], sh.ri[par][w]);
        }
        if (hi == wi && wi != INT_MAX) {  // the winning list: its head is entry j, and it moves on
            top_ids[(size_t)b * k + j] = hi;
            top_lps[(size_t)b * k + j] = (float)((double)hv - lse);
            ++p;
            hv = p < k ? cv[t * k + p] : -INFINITY;
            hi = p < k ? ci[t * k + p] : INT_MAX;
        }
    }
}

// module-owned workspace of hpa_top_logprobs (grown on demand, kept for the process)
void* g_top_ws = nullptr;
size_t g_top_ws_bytes = 0;
}  // namespace

extern "C" {

int hpa_top_logprobs_slices(int rows, int V, int num_cus) {
    if (rows <= 0 || V <= 0) return 0;
    if (num_cus <= 0) num_cus = 256;
    const int nq = V >> 2;
    // a slice is a wave's: about sixteen waves per CU over the launch, no slice
    // under one 16-byte load per lane, no more than the final kernel merges in one
    // wave -- and none over what a wave holds in registers, whatever that takes
    int s = (16 * num_cus + rows - 1) / rows;
    const int by_size = (nq + 63) / 64;
    if (s > by_size) s = by_size;
    if (s > kTsOneWave) s = kTsOneWave;
    const int smin = (nq + kTsSliceQ - 1) / kTsSliceQ;
    if (s < smin) s = smin;
    return s < 1 ? 1 : s;
}

int hpa_top_logprobs_workspace(int rows, int V, int k, size_t* bytes) {
    HPA_REQUIRE(bytes && rows > 0 && V > 0 && k >= 1 && k <= HPA_TOP_LOGPROBS_MAX, "top_logprobs_workspace: bad arguments");
    // enough for every launch of n <= rows rows: n * slices(n) is at most
    // rows * (fewest slices of V) where the register limit sets the count, and
    // under both 16 CUs' worth of waves + n and 64 n where the occupancy target does
    const size_t ncu = hpa::num_cus() > 0 ? (size_t)hpa::num_cus() : 256;
    const size_t smin = (size_t)(((V >> 2) + kTsSliceQ - 1) / kTsSliceQ);
    size_t cells = (size_t)rows * (smin ? smin : 1);
    const size_t by_cus = 16 * ncu + rows, by_wave = (size_t)rows * kTsOneWave;
    const size_t other = by_cus < by_wave ? by_cus : by_wave;
    if (other > cells) cells = other;
    *bytes = top_ws_bytes(cells, (size_t)k);
    return 0;
}

int hpa_top_logprobs_ws(const float* logits, int rows, int V, int k, const int* active, const int* targets,
                        int* top_ids, float* top_lps, float* target_lp, float* lse, void* ws, size_t ws_bytes,
                        int slices) {
    HPA_REQUIRE(k >= 1 && k <= HPA_TOP_LOGPROBS_MAX && k <= V, "top_logprobs: k outside [1, min(V, HPA_TOP_LOGPROBS_MAX)]");
    HPA_REQUIRE(logits && top_ids && top_lps && ws && rows > 0 && rows <= 65535, "top_logprobs: bad arguments");
    HPA_REQUIRE(!target_lp || targets, "top_logprobs: target_lp without targets");
    HPA_REQUIRE(((size_t)logits & 3) == 0 && ((size_t)ws & 7) == 0, "top_logprobs: unaligned buffers");
    const int S = slices > 0 ? slices : hpa_top_logprobs_slices(rows, V, hpa::num_cus());
    // every slice in a wave's registers, one lane of the final workgroup per slice
    HPA_REQUIRE(((V >> 2) + S - 1) / S <= kTsSliceQ && S <= kTsMaxSlices, "top_logprobs: slices too few for V, or too many");
    const size_t cells = (size_t)rows * S;
    HPA_REQUIRE(ws_bytes >= top_ws_bytes(cells, (size_t)k), "top_logprobs: workspace too small");
    const TopWs w = top_ws_cut(ws, cells, (size_t)k);
    top_slice_kernel<<<dim3((S + kTsWaves - 1) / kTsWaves, rows), kTsThreads, 0, hpa_stream()>>>(
        logits, V, k, S, active, w.sum, w.mx, w.cv, w.ci);
    HPA_LAUNCH_CHECK();
    top_final_kernel<<<rows, S <= kTsOneWave ? 64 : kTsThreads, (size_t)S * k * 8, hpa_stream()>>>(
        logits, V, k, S, active, targets, w.sum, w.mx, w.cv, w.ci, top_ids, top_lps, target_lp, lse);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_top_logprobs(const float* logits, int rows, int V, int k, const int* active, const int* targets, int* top_ids,
                     float* top_lps, float* target_lp, float* lse) {
    HPA_REQUIRE(k >= 1 && k <= HPA_TOP_LOGPROBS_MAX && k <= V, "top_logprobs: k outside [1, min(V, HPA_TOP_LOGPROBS_MAX)]");
    HPA_REQUIRE(logits && top_ids && top_lps && rows > 0 && rows <= 65535, "top_logprobs: bad arguments");
    size_t need = 0;
    if (hpa_top_logprobs_workspace(rows, V, k, &need)) return 1;
    if (need > g_top_ws_bytes) {  // queued launches may still read the old one (not while a graph is captured)
        HPA_CHECK(hipStreamSynchronize(hpa_stream()));
        if (g_top_ws) HPA_CHECK(hipFree(g_top_ws));
        g_top_ws = nullptr;
        g_top_ws_bytes = 0;
        HPA_CHECK(hipMalloc(&g_top_ws, need));
        g_top_ws_bytes = need;
    }
    return hpa_top_logprobs_ws(logits, rows, V, k, active, targets, top_ids, top_lps, target_lp, lse, g_top_ws,
                               g_top_ws_bytes, 0);
}

}  // extern "C"
