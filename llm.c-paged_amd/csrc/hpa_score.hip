// hpa_score.hip -- per-token log-probabilities.
//
// hpa_score_final   combines the row partials of a SCORE GEMM (HPA_FEPI_SCORE,
//                   hpa_gemm_body.h: per 16-column tile and row the maximum m_t,
//                   s_t = sum expf(v - m_t), the target's logit, the first
//                   maximum's column) into log-sum-exp, the target's
//                   log-probability, the greedy id and its log-probability.
// hpa_logprob_rows  the same quantity for a token the decode step just chose,
//                   from the step's dense [B][V] logits.
//
// Both sum in double in a fixed order (every thread its items in increasing
// order; the threads' sums meet in a fixed tree), so a launch repeats bit for
// bit.  hpa_logprob_rows runs one workgroup of 1024 threads per row,
// hpa_score_final one of 1024 per four rows.
//
// Error of logprob against the float64 log-softmax of the same fp32 logits
// (hpa_score_final; DESIGN.md "Scoring"): s_t carries at most 5 dependent
// fp32 additions of terms in [0, 1] (bounded as 16: 16 * 2^-24), each term an
// exp good to 1 ulp of v_exp_f32 plus the rounding of its argument's product
// with log2 e (|d| e^d 2^-24 <= 2.2e-8 of the largest term, 16 terms): a
// relative error below 9.5e-7 + 1.2e-7 + 3.5e-7 = 1.5e-6 of S, hence of log S
// in absolute terms; the double combine adds nothing visible; lse and the
// difference are each rounded to fp32 once: 2 * 2^-24 * max(|lse|, |target
// logit|).  Within 4e-6 + 2^-22 * max(|lse|, |x_t|).  hpa_logprob_rows: expf
// (<= 2 ulp) terms added in double: 2.4e-7 + the two roundings.
#include <math.h>

#include "hpa_internal.h"

namespace {
constexpr int kScThreads = 1024;  // hpa_score_final: four rows per workgroup
constexpr int kLrThreads = 1024;  // hpa_logprob_rows: one row (201 KB at V = 50257) per workgroup

struct LrShared {
    float mx[kLrThreads / 64];
    double sum[kLrThreads];
};

// Four rows per workgroup: thread t takes row (t & 3) and tile lane (t >> 2),
// so the four lanes of a tile read one 64-byte run of part[tile][Mp] and a
// wave reads 16 tiles' runs (with one row per workgroup every load took 16
// bytes out of a 16 KiB stride; profiles/EXPERIMENTS.md "Scoring").
// One pass: every thread folds its tiles t>>2, t>>2 + 256, ... in increasing
// order into a running (maximum m, S = sum s_t exp(m_t - m)) in double, then
// the 256 tile lanes of a row meet in a fixed LDS tree (strides 512 .. 4).
// 16 waves per workgroup with four loads each in flight: at 4 waves the
// launch was bound by latency (2.1 TB/s of partials, profiles/EXPERIMENTS.md).
struct SfShared {
    double S[kScThreads];
    float m[kScThreads], tl[kScThreads];
    int arg[kScThreads];
};

// (m, S, arg) <- combined with (m2, S2, arg2): the common maximum (lowest column on
// ties).  One exp per merge and no branch around it: the smaller side is scaled by
// e = exp(-|m - m2|) (a side at -inf has sum 0: e = 0, or 1 when both are)
__device__ __forceinline__ void lse_merge(float& m, double& S, int& arg, float m2, double S2, int arg2) {
    const double e = m2 == m ? 1.0 : exp(-fabs((double)m - (double)m2));
    const bool up = m2 > m;
    S = up ? S * e + S2 : S + S2 * e;
    if (up || (m2 == m && arg2 < arg)) arg = arg2;
    if (up) m = m2;
}

__global__ __launch_bounds__(kScThreads) void score_final_kernel(const float4* __restrict__ part, int ntiles, int Mp,
                                                                 int M, float* __restrict__ logprob,
                                                                 float* __restrict__ lse, int* __restrict__ top_id,
                                                                 float* __restrict__ top_logprob) {
    __shared__ SfShared sh;
    const int b = blockIdx.x * 4 + (threadIdx.x & 3);  // < Mp: the grid covers ceil(M / 4) row quads, Mp % 16 == 0
    float m = -INFINITY, tl = -INFINITY;
    double S = 0.0;
    int arg = 0x7fffffff;
    constexpr int TL = kScThreads / 4;  // tile lanes
    int t = threadIdx.x >> 2;
    for (; t + 3 * TL < ntiles; t += 4 * TL) {  // four loads in flight
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = part[(size_t)(t + u * TL) * Mp + b];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            lse_merge(m, S, arg, q[u].x, (double)q[u].y, __float_as_int(q[u].w));
            tl = fmaxf(tl, q[u].z);  // at most one tile holds the target's logit: every other slot is -inf
        }
    }
    for (; t < ntiles; t += TL) {
        const float4 q = part[(size_t)t * Mp + b];
        lse_merge(m, S, arg, q.x, (double)q.y, __float_as_int(q.w));
        tl = fmaxf(tl, q.z);
    }
    sh.m[threadIdx.x] = m;
    sh.S[threadIdx.x] = S;
    sh.arg[threadIdx.x] = arg;
    sh.tl[threadIdx.x] = tl;
    __syncthreads();
    for (int o = kScThreads / 2; o >= 4; o >>= 1) {  // o % 4 == 0: partners share the row
        if ((int)threadIdx.x < o) {
            lse_merge(m, S, arg, sh.m[threadIdx.x + o], sh.S[threadIdx.x + o], sh.arg[threadIdx.x + o]);
            tl = fmaxf(tl, sh.tl[threadIdx.x + o]);
            sh.m[threadIdx.x] = m;
            sh.S[threadIdx.x] = S;
            sh.arg[threadIdx.x] = arg;
            sh.tl[threadIdx.x] = tl;
        }
        __syncthreads();
    }
    if (threadIdx.x < 4 && b < M) {
        const double l = (double)m + log(S);
        if (lse) lse[b] = (float)l;
        if (logprob) logprob[b] = tl == -INFINITY ? 0.0f : (float)((double)tl - l);
        if (top_id) top_id[b] = arg == 0x7fffffff ? 0 : arg;
        if (top_logprob) top_logprob[b] = (float)((double)m - l);
    }
}

// two passes over the row (the second from L2): the maximum, then the sum of
// expf(x - max) in double, thread t its elements t, t + 1024, ... in increasing
// order, the threads' sums in a fixed LDS tree
__global__ __launch_bounds__(kLrThreads) void logprob_rows_kernel(const float* __restrict__ logits, int V,
                                                                  const int* __restrict__ ids,
                                                                  const int* __restrict__ active,
                                                                  float* __restrict__ logprob) {
    __shared__ LrShared sh;
    const int b = blockIdx.x;
    if (active && active[b] <= 0) return;  // row left as it is
    const float* lg = logits + (size_t)b * V;
    float mx = -INFINITY;
#pragma unroll 8
    for (int i = threadIdx.x; i < V; i += kLrThreads) mx = fmaxf(mx, lg[i]);
    mx = hpa::wave_max(mx);
    if ((threadIdx.x & 63) == 0) sh.mx[threadIdx.x >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kLrThreads / 64; ++k) mx = fmaxf(mx, sh.mx[k]);
    double s = 0.0;
#pragma unroll 8
    for (int i = threadIdx.x; i < V; i += kLrThreads) s += (double)expf(lg[i] - mx);
    sh.sum[threadIdx.x] = s;
    __syncthreads();
    for (int o = kLrThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh.sum[threadIdx.x] += sh.sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int id = ids[b];
        logprob[b] = id < 0 || id >= V ? 0.0f : (float)((double)lg[id] - ((double)mx + log(sh.sum[0])));
    }
}
}  // namespace

extern "C" {

int hpa_score_workspace(int N, int chunk_rows, size_t* floats) {
    HPA_REQUIRE(floats && N > 0 && chunk_rows > 0 && chunk_rows % 16 == 0,
                "score_workspace: N > 0 and chunk_rows a positive multiple of 16");
    *floats = (size_t)((N + 15) / 16) * (size_t)chunk_rows * 4;
    return 0;
}

int hpa_score_final(const float* part, int ntiles, int Mp, int M, float* logprob, float* lse, int* top_id,
                    float* top_logprob) {
    HPA_REQUIRE(part && ((size_t)part & 15) == 0 && ntiles > 0 && M > 0 && Mp >= M && Mp % 16 == 0,
                "score_final: bad arguments");
    score_final_kernel<<<(M + 3) / 4, kScThreads, 0, hpa_stream()>>>(reinterpret_cast<const float4*>(part), ntiles, Mp, M,
                                                                     logprob, lse, top_id, top_logprob);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_logprob_rows(const float* logits, int B, int V, const int* ids, const int* active, float* logprob) {
    HPA_REQUIRE(logits && ids && logprob && B > 0 && V > 0, "logprob_rows: bad arguments");
    logprob_rows_kernel<<<B, kLrThreads, 0, hpa_stream()>>>(logits, V, ids, active, logprob);
    HPA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
