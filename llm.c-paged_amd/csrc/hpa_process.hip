// hpa_process.hip -- logit processors on the device: repetition, presence
// and frequency penalties and a sparse logit bias per row (the rules are in
// hip_paged_attn.h), and the token history / count table they read.
//
// hpa_logits_process   one pass over the raw [B][V] logits and the uint16
//                      counts: grid (slice, row), 256 threads, 16-byte loads of
//                      logits and 8-byte loads of counts, kLpLoads of each in
//                      flight per lane.  Rows are only 4-byte (counts: 2-byte)
//                      aligned, so every row peels its own head and tail
//                      (hpa_sample.hip's walk).  The bias list is sparse: the
//                      slice's columns that carry a bias are marked in an LDS
//                      bitmap, one nibble per 16-byte load, and a marked column
//                      looks its value up in the list (also in LDS).
//                      Every slice leaves a (max, argmax) partial in the
//                      layout hpa_argmax_final reads.
// hpa_token_record     history[seq][pos] = tok and an integer atomic add on
//                      the count (order-independent, so repeatable)
// hpa_token_recount    one row of counts rebuilt from the history
//
// Counts are uint16 pairs inside 32-bit words: the add is 1 << 16 * (index & 1)
// on the word.  A count never passes max_ctx <= 65535, so no carry crosses
// into the neighbouring count (which may belong to the next row).
#include <limits.h>
#include <math.h>

#include "hpa_internal.h"

namespace {
constexpr int kLpThreads = 256;
constexpr int kLpWaves = kLpThreads / 64;
constexpr int kLpLoads = 4;            // 16-byte logit loads (and 8-byte count loads) in flight per lane
constexpr int kLpSliceBits = 65536;    // bitmap bits per slice: 8 KiB of LDS
constexpr int kLpMinSlice = 1024;      // columns: one 16-byte load per lane of a workgroup

struct LpShared {
    unsigned bits[kLpSliceBits / 32];
    int ids[HPA_LOGIT_BIAS_MAX];
    float vals[HPA_LOGIT_BIAS_MAX];
    float red_v[kLpWaves];
    int red_i[kLpWaves];
};

// the larger value wins, then the lower column
__device__ __forceinline__ void lp_take(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

__global__ __launch_bounds__(kLpThreads) void logits_process_kernel(
    const float* __restrict__ logits, int V, const unsigned short* __restrict__ counts, const float* __restrict__ rep,
    const float* __restrict__ pres, const float* __restrict__ freq, const int* __restrict__ bias_ids,
    const float* __restrict__ bias_vals, const int* __restrict__ bias_n, const int* __restrict__ active,
    float* __restrict__ out, float* __restrict__ part, int Mp) {
    __shared__ LpShared sh;
    const int s = blockIdx.x, S = gridDim.x, b = blockIdx.y, t = threadIdx.x;
    if (active && active[b] <= 0) return;  // row left as it is: processed row and partials
    const float* lg = logits + (size_t)b * V;
    const unsigned short* cn = counts + (size_t)b * V;
    float* o = out ? out + (size_t)b * V : nullptr;
    // head scalars, nq aligned float4s from lg + head, tail scalars from tail0
    const int head = min(V, (int)((4u - (unsigned)(((size_t)lg >> 2) & 3u)) & 3u));
    const int nq = (V - head) >> 2, tail0 = head + 4 * nq;
    const int Q = (nq + S - 1) / S;
    const int qlo = min(nq, s * Q), qhi = min(nq, qlo + Q);
    const int c0 = s == 0 ? 0 : head + 4 * qlo;      // this slice's columns [c0, c1): slice 0 takes the
    const int c1 = s == S - 1 ? V : head + 4 * qhi;  // head, the last slice the tail
    const int bit0 = head + 4 * qlo - 4;             // column -> bitmap bit: a float4's four bits share a nibble
    const bool c_al = (((size_t)(cn + head)) & 7) == 0;          // 8-byte count loads
    const bool o_al = o && (((size_t)(o + head)) & 15) == 0;     // 16-byte stores
    const float r = rep[b], p = pres[b], f = freq[b];

    const int nb = bias_n ? min(max(bias_n[b], 0), HPA_LOGIT_BIAS_MAX) : 0;
    if (nb > 0) {  // wave-uniform
        const int nwords = (4 * (qhi - qlo) + 8 + 31) >> 5;
        for (int i = t; i < nwords; i += kLpThreads) sh.bits[i] = 0;
        __syncthreads();
        for (int i = t; i < nb; i += kLpThreads) {
            const int id = bias_ids[(size_t)b * HPA_LOGIT_BIAS_MAX + i];
            sh.ids[i] = id;
            sh.vals[i] = bias_vals[(size_t)b * HPA_LOGIT_BIAS_MAX + i];
            if (id >= c0 && id < c1) atomicOr(&sh.bits[(id - bit0) >> 5], 1u << ((id - bit0) & 31));
        }
        __syncthreads();
    }
    auto bias_of = [&](int col) {  // rare: at most HPA_LOGIT_BIAS_MAX columns of a row
        for (int i = 0; i < nb; ++i)
            if (sh.ids[i] == col) return sh.vals[i];
        return 0.f;
    };
    // fp32, every step rounded on its own (no contraction): exact for r = 1, f = p = 0
    auto one = [&](float x, unsigned c, bool biased, int col) {
        if (c > 0) x = x > 0.f ? __fdiv_rn(x, r) : __fmul_rn(x, r);
        x = __fsub_rn(__fsub_rn(x, __fmul_rn(f, (float)c)), c > 0 ? p : 0.f);
        if (biased) x = __fadd_rn(x, bias_of(col));
        return x;
    };
    auto scalar = [&](int col, float& bv, int& bi) {
        const bool biased = nb > 0 && ((sh.bits[(col - bit0) >> 5] >> ((col - bit0) & 31)) & 1u);
        const float y = one(lg[col], cn[col], biased, col);
        if (o) o[col] = y;
        lp_take(bv, bi, y, col);
    };

    float bv = -INFINITY;
    int bi = INT_MAX;
    if (s == 0 && t < head) scalar(t, bv, bi);
    const float4* lq = reinterpret_cast<const float4*>(lg + head);
    const uint2* cq = reinterpret_cast<const uint2*>(cn + head);
    for (int q0 = qlo; q0 < qhi; q0 += kLpLoads * kLpThreads) {
        float4 v[kLpLoads];
        uint2 cw[kLpLoads];
#pragma unroll
        for (int u = 0; u < kLpLoads; ++u) {
            const int q = q0 + t + u * kLpThreads;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            cw[u] = make_uint2(0u, 0u);
            if (q < qhi) {
                v[u] = lq[q];
                if (c_al) {
                    cw[u] = cq[q];
                } else {
                    const unsigned short* c4 = cn + head + 4 * q;
                    cw[u] = make_uint2(c4[0] | ((unsigned)c4[1] << 16), c4[2] | ((unsigned)c4[3] << 16));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kLpLoads; ++u) {
            const int q = q0 + t + u * kLpThreads;
            if (q >= qhi) continue;
            const int col = head + 4 * q;
            unsigned nib = 0;
            if (nb > 0) nib = (sh.bits[(col - bit0) >> 5] >> ((col - bit0) & 31)) & 15u;
            float4 y;
            y.x = one(v[u].x, cw[u].x & 0xffffu, nib & 1u, col);
            y.y = one(v[u].y, cw[u].x >> 16, nib & 2u, col + 1);
            y.z = one(v[u].z, cw[u].y & 0xffffu, nib & 4u, col + 2);
            y.w = one(v[u].w, cw[u].y >> 16, nib & 8u, col + 3);
            if (o_al) {
                *reinterpret_cast<float4*>(o + col) = y;
            } else if (o) {
                o[col] = y.x;
                o[col + 1] = y.y;
                o[col + 2] = y.z;
                o[col + 3] = y.w;
            }
            lp_take(bv, bi, y.x, col);
            lp_take(bv, bi, y.y, col + 1);
            lp_take(bv, bi, y.z, col + 2);
            lp_take(bv, bi, y.w, col + 3);
        }
    }
    if (s == S - 1 && t < V - tail0) scalar(tail0 + t, bv, bi);
    if (!part) return;

    // fixed-order reduction: wave butterfly, then the four waves in order
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const float v2 = __shfl_xor(bv, w, 64);
        const int i2 = __shfl_xor(bi, w, 64);
        lp_take(bv, bi, v2, i2);
    }
    if ((t & 63) == 0) {
        sh.red_v[t >> 6] = bv;
        sh.red_i[t >> 6] = bi;
    }
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < kLpWaves; ++k) lp_take(bv, bi, sh.red_v[k], sh.red_i[k]);
        part[((size_t)s * Mp + b) * 2] = bv;  // a slice without a finite value: (-inf, INT_MAX), never taken
        part[((size_t)s * Mp + b) * 2 + 1] = __int_as_float(bi);
    }
}

__device__ __forceinline__ void count_add(unsigned short* counts, size_t e) {
    // counts is 4-byte aligned (checked by the launchers)
    atomicAdd(reinterpret_cast<unsigned*>(counts) + (e >> 1), 1u << (16 * (unsigned)(e & 1)));
}

__global__ __launch_bounds__(256) void token_record_kernel(int* __restrict__ history, int max_ctx,
                                                           unsigned short* __restrict__ counts, int V, int B,
                                                           const int* __restrict__ from_pos,
                                                           const int* __restrict__ seq, const int* __restrict__ pos,
                                                           const int* __restrict__ tok, int R) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int b = seq ? seq[i] : i, p = pos[i], x = tok[i];
    if (b < 0 || b >= B || p < 0 || p >= max_ctx || x < 0 || x >= V) return;  // nothing outside the tables
    history[(size_t)b * max_ctx + p] = x;
    if (p >= from_pos[b]) count_add(counts, (size_t)b * V + x);
}

constexpr int kRcThreads = 1024;
__global__ __launch_bounds__(kRcThreads) void token_recount_kernel(const int* __restrict__ history, int max_ctx,
                                                                   unsigned short* __restrict__ counts, int V,
                                                                   int seq, int from, int n) {
    unsigned short* row = counts + (size_t)seq * V;
    for (int i = threadIdx.x; i < V; i += kRcThreads) row[i] = 0;
    __threadfence();  // one workgroup: its stores have reached L2, where the atomics run, before the barrier
    __syncthreads();
    for (int p = from + (int)threadIdx.x; p < n; p += kRcThreads) {
        const int x = history[(size_t)seq * max_ctx + p];
        if (x >= 0 && x < V) count_add(counts, (size_t)seq * V + x);
    }
}
}  // namespace

int hpa_logits_process_slices(int B, int V, int num_cus) {
    if (B <= 0 || V <= 0) return 0;
    if (num_cus <= 0) num_cus = 256;
    // about four workgroups per CU over the whole launch, no slice under one
    // 16-byte load per lane, none over the LDS bitmap
    int s = (4 * num_cus + B - 1) / B;
    const int smax = V / kLpMinSlice;
    if (s > smax) s = smax;
    const int smin = (V + (kLpSliceBits - 64) - 1) / (kLpSliceBits - 64);
    if (s < smin) s = smin;
    return s < 1 ? 1 : s;
}

int hpa_logits_process(const float* logits, int B, int V, const unsigned short* counts, const float* repetition,
                       const float* presence, const float* frequency, const int* bias_ids, const float* bias_values,
                       const int* bias_n, const int* active, float* processed, float* part, int Mp, int slices) {
    HPA_REQUIRE(logits && counts && repetition && presence && frequency && B > 0 && B <= 65535 && V > 0,
                "logits_process: bad arguments");
    HPA_REQUIRE(((size_t)logits & 3) == 0 && ((size_t)counts & 1) == 0 && ((size_t)processed & 3) == 0,
                "logits_process: unaligned buffers");
    HPA_REQUIRE(!bias_n || (bias_ids && bias_values), "logits_process: bias_n without the bias tables");
    HPA_REQUIRE(!part || Mp >= B, "logits_process: Mp < B");
    if (slices <= 0) slices = hpa_logits_process_slices(B, V, hpa::num_cus());
    // the longest slice (rows' heads differ: at most (V >> 2) float4s) fits the bitmap
    const int Q = ((V >> 2) + slices - 1) / slices;
    HPA_REQUIRE(slices >= 1 && 4 * (long long)Q + 8 <= kLpSliceBits, "logits_process: slices too few for V");
    logits_process_kernel<<<dim3(slices, B), kLpThreads, 0, hpa_stream()>>>(
        logits, V, counts, repetition, presence, frequency, bias_ids, bias_values, bias_n, active, processed, part, Mp);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_token_record(int* history, int max_ctx, unsigned short* counts, int V, int B, const int* from_pos,
                     const int* seq, const int* pos, const int* tok, int R) {
    HPA_REQUIRE(history && counts && from_pos && pos && tok && max_ctx > 0 && max_ctx <= 65535 && V > 0 && B > 0 &&
                    R >= 0 && ((size_t)counts & 3) == 0,
                "token_record: bad arguments");
    if (R == 0) return 0;
    token_record_kernel<<<(R + 255) / 256, 256, 0, hpa_stream()>>>(history, max_ctx, counts, V, B, from_pos, seq, pos,
                                                                    tok, R);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_token_recount(const int* history, int max_ctx, unsigned short* counts, int V, int seq, int from, int n) {
    HPA_REQUIRE(history && counts && max_ctx > 0 && max_ctx <= 65535 && V > 0 && seq >= 0 && from >= 0 &&
                    n <= max_ctx && ((size_t)counts & 3) == 0,
                "token_recount: bad arguments");
    token_recount_kernel<<<1, kRcThreads, 0, hpa_stream()>>>(history, max_ctx, counts, V, seq, from, n);
    HPA_LAUNCH_CHECK();
    return 0;
}
