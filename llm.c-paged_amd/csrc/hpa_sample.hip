// hpa_sample.hip -- temperature / top-k / top-p sampling, per row, on the
// device (hpa_sample_filtered; the rules are in hip_paged_attn.h).
//
// One workgroup of 16 waves per row.  The row (V fp32 logits, 201 KB at
// V = 50257) is never sorted and never staged: every pass streams it from L2
// with 16-byte loads (head and tail peeled, rows are only 4-byte aligned).
//
//   pass 1     max (lowest index), min                        -> greedy rows end here
//   top-k      radix select of the k-th largest order-preserving key: four
//              8-bit digits, one 256-bin count histogram in LDS per digit
//   top-p      the same descent over the top-k set with a probability-mass
//              histogram beside the counts; the tie group at the cut is
//              resolved by count (equal logits have equal mass)
//   draw       every wave sums the kept mass of a contiguous part of the row;
//              the part where the running sum passes the coin is scanned
//              again with wave prefix sums
//
// Masses are fixed point: w_i = (uint64) (exp2((x_i - max) * (log2 e / T)) * 2^s), s
// chosen so that V of them cannot overflow (two multiplies, one exp2 and one
// convert per element; the scale stays outside the exponent, whose rounding
// error grows with its magnitude).  Integer sums are exact, so histogram
// atomics, wave reductions and the per-part combine give the same totals in
// any order: two launches on the same inputs return the same ids, and the
// cdf test  running / total > u  is the integer test  running * 2^24 > total * j
// (u = j / 2^24).  The quantisation is below 2^-41 of the total per term.
#include <limits.h>
#include <math.h>

#include "hpa_internal.h"

namespace {
typedef unsigned long long u64;
constexpr int kSfThreads = 1024;
constexpr int kSfWaves = kSfThreads / 64;
constexpr int kSfSegs = kSfWaves + 2;  // head scalars, one part per wave, tail scalars

struct SfShared {
    unsigned cnt[256];
    u64 mass[256];
    float red_max[kSfWaves], red_min[kSfWaves];
    int red_arg[kSfWaves];
    unsigned seg_ties[kSfSegs];
    u64 seg_mass[kSfSegs];
    unsigned digit, bin_count, c_above;
    u64 m_above, target;
    int pick;
    unsigned cut_bits;
};

// order-preserving key: a > b  <=>  key(a) > key(b)   (no NaNs; -0 is read as +0)
__device__ __forceinline__ unsigned sf_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sf_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

struct SfRow {
    const float* lg;
    int V, head, nq, tail0;  // head scalars, nq aligned float4s from lg + head, tail scalars from tail0
    float mx, c, scale;  // c = log2(e) / T (finite), scale = 2^s
    __device__ __forceinline__ u64 w(float x) const { return (u64)(exp2f((x - mx) * c) * scale); }
    __device__ __forceinline__ const float4* q4() const { return reinterpret_cast<const float4*>(lg + head); }
};

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// kSfLoads 16-byte loads per lane are issued before the first is used.  (Eight
// measured the same as two and as one: with one workgroup per row a pass is
// bound by instruction issue, about 0.33 us per instruction per element at
// V = 50257, not by load latency; profiles/r9/sample_filtered.txt.)
constexpr int kSfLoads = 8;
__device__ __forceinline__ void sf_load(const float4* q4, int q, int stride, int qend, float4 (&v)[kSfLoads]) {
#pragma unroll
    for (int u = 0; u < kSfLoads; ++u) {
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q + u * stride < qend) v[u] = q4[q + u * stride];
    }
}

// f(x, index, valid) over the whole row, in no particular order, with
// wave-uniform trip counts (f may use wave intrinsics); -0 arrives as +0
template <typename F>
__device__ __forceinline__ void sf_foreach(const SfRow& r, F&& f) {
    const int t = threadIdx.x;
    const float4* q4 = r.q4();
    for (int q0 = 0; q0 < r.nq; q0 += kSfLoads * kSfThreads) {
        float4 v[kSfLoads];
        sf_load(q4, q0 + t, kSfThreads, r.nq, v);
#pragma unroll
        for (int u = 0; u < kSfLoads; ++u) {
            const int q = q0 + t + u * kSfThreads;
            const bool ok = q < r.nq;
            const int i = r.head + 4 * q;
            f(v[u].x + 0.f, i, ok);
            f(v[u].y + 0.f, i + 1, ok);
            f(v[u].z + 0.f, i + 2, ok);
            f(v[u].w + 0.f, i + 3, ok);
        }
    }
    if (t < 64) {  // the at most 6 unaligned head and tail elements, wave 0
        const int ne = r.head + (r.V - r.tail0);
        const bool ok = t < ne;
        const int i = t < r.head ? t : r.tail0 + (t - r.head);
        f(ok ? r.lg[i] + 0.f : 0.f, i, ok);
    }
}

// one element into the digit histograms.  The lanes that share the first
// matching lane's digit are combined into one atomic when they are many
// (peaked digit distributions serialise same-address LDS atomics otherwise).
template <bool MASS>
__device__ __forceinline__ void sf_hist_add(SfShared& sh, bool match, unsigned d, u64 wv) {
    const u64 rem = __ballot(match);
    if (rem == 0) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)rem) - 1;
    const unsigned d0 = __shfl(d, leader, 64);
    const bool in = match && d == d0;
    const u64 grp = __ballot(in);
    if (__popcll(grp) >= 8) {
        u64 ws = 0;
        if (MASS) ws = wave_sum_u64(in ? wv : 0);
        if (lane == leader) {
            atomicAdd(&sh.cnt[d0], (unsigned)__popcll(grp));
            if (MASS) atomicAdd(&sh.mass[d0], ws);
        }
        match = match && !in;
    }
    if (match) {
        atomicAdd(&sh.cnt[d], 1u);
        if (MASS) atomicAdd(&sh.mass[d], wv);
    }
}

// wave 0: the highest bin at which the running count (or mass), bins taken
// from 255 down, reaches `need`; c_above / m_above gain what lies above it
template <bool MASS>
__device__ __forceinline__ void sf_walk(SfShared& sh, int lane, u64 need) {
    unsigned c[4], ct = 0;
    u64 m[4], mt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int bin = 255 - 4 * lane - i;
        c[i] = sh.cnt[bin];
        ct += c[i];
        m[i] = MASS ? sh.mass[bin] : 0;
        mt += m[i];
    }
    unsigned ci = ct;
    u64 mi = mt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned uc = __shfl_up(ci, o, 64);
        const u64 um = MASS ? __shfl_up(mi, o, 64) : 0;
        if (lane >= o) {
            ci += uc;
            mi += um;
        }
    }
    const u64 hit = __ballot(MASS ? mi >= need : (u64)ci >= need);
    const int f = hit ? __ffsll((long long)hit) - 1 : 63;
    if (lane == f) {
        unsigned ce = ci - ct;
        u64 me = mi - mt;
        int i = 0;
        for (; i < 3; ++i) {
            if (MASS ? me + m[i] >= need : (u64)(ce + c[i]) >= need) break;
            ce += c[i];
            me += m[i];
        }
        sh.digit = 255 - 4 * lane - i;
        sh.bin_count = c[i];
        sh.c_above += ce;
        if (MASS) sh.m_above += me;
    }
}

// Radix descent over the canonical order (key descending).
//   MASS = false: the key of the `kneed`-th largest element of the row.
//   MASS = true:  over the top-k set (keys above Kk, plus tieK elements equal
//                 to Kk; the whole row without haveK), the key at which the
//                 running mass reaches ceil(P * total).
// Returns the key; c_gt / m_gt: count and mass strictly above it; bin: the
// number of set elements equal to it; target: the mass to reach.
template <bool MASS>
__device__ __forceinline__ unsigned sf_descend(SfShared& sh, const SfRow& r, bool haveK, unsigned Kk, unsigned tieK,
                                               unsigned kneed, float P, unsigned& c_gt, u64& m_gt, unsigned& bin,
                                               u64& target) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) {
        sh.c_above = 0;
        sh.m_above = 0;
    }
    unsigned prefix = 0;
    for (int L = 0; L < 4; ++L) {
        const int sd = 24 - 8 * L;
        const unsigned himask = L == 0 ? 0u : 0xffffffffu << (sd + 8);
        if (t < 256) {
            sh.cnt[t] = 0;
            sh.mass[t] = 0;
        }
        __syncthreads();
        sf_foreach(r, [&](float x, int, bool ok) {
            const unsigned key = sf_key(x);
            bool match = ok && ((key ^ prefix) & himask) == 0;
            if (MASS && haveK) match = match && key > Kk;
            const u64 wv = (MASS && match) ? r.w(x) : 0;
            sf_hist_add<MASS>(sh, match, (key >> sd) & 255u, wv);
        });
        __syncthreads();
        if (MASS && haveK && t == 0 && ((Kk ^ prefix) & himask) == 0) {  // the capped tie group at the top-k cut
            sh.cnt[(Kk >> sd) & 255u] += tieK;
            sh.mass[(Kk >> sd) & 255u] += (u64)tieK * r.w(sf_unkey(Kk));
        }
        if (MASS && haveK) __syncthreads();
        if (w == 0) {
            u64 need;
            if (MASS) {
                u64 tg;
                if (L == 0) {
                    u64 s = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) s += sh.mass[4 * lane + i];
                    s = wave_sum_u64(s);
                    tg = (u64)ceil((double)P * (double)s);
                    tg = tg < 1 ? 1 : tg > s ? s : tg;
                } else {
                    tg = sh.target;
                }
                need = tg - sh.m_above;
                sf_walk<true>(sh, lane, need);
                if (L == 0 && lane == 0) sh.target = tg;
            } else {
                need = (u64)(kneed - sh.c_above);
                sf_walk<false>(sh, lane, need);
            }
        }
        __syncthreads();
        prefix |= sh.digit << sd;
    }
    c_gt = sh.c_above;
    m_gt = sh.m_above;
    bin = sh.bin_count;
    target = sh.target;
    __syncthreads();  // the next descent resets these
    return prefix;
}

__global__ __launch_bounds__(kSfThreads) void sample_filtered_kernel(
    const float* __restrict__ logits, int V, const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, unsigned long long* __restrict__ state, int* __restrict__ next,
    int* __restrict__ tokens, int* __restrict__ pos, const int* __restrict__ active, int* __restrict__ n_kept,
    float* __restrict__ cut_out, int shift) {
    __shared__ SfShared sh;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (active && active[b] <= 0) return;  // row left as it is (its RNG state too)
    SfRow r;
    r.lg = logits + (size_t)b * V;
    r.V = V;
    r.head = min(V, (int)((4u - (unsigned)(((size_t)r.lg >> 2) & 3u)) & 3u));
    r.nq = (V - r.head) >> 2;
    r.tail0 = r.head + 4 * r.nq;
    r.scale = (float)(1ull << shift);

    // per-row parameters, sanitised so that nothing below can leave the row
    float T = temperature[b];
    if (!(T >= 0.f) || isinf(T)) T = 1.f;
    int k = top_k[b];
    if (k < 0) k = 0;
    float P = top_p[b];
    if (!(P > 0.f && P <= 1.f)) P = 1.f;
    unsigned long long st = state[b];
    const u64 coin = hpa::xorshift_u32(st) >> 8;  // u = coin / 2^24

    // pass 1: max (lowest index on ties) and min
    float mx = -INFINITY, mn = INFINITY;
    int am = INT_MAX;
    sf_foreach(r, [&](float x, int i, bool ok) {
        if (ok) {
            if (x > mx || (x == mx && i < am)) {
                mx = x;
                am = i;
            }
            mn = fminf(mn, x);
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ox = __shfl_xor(mx, o, 64);
        const int oi = __shfl_xor(am, o, 64);
        if (ox > mx || (ox == mx && oi < am)) {
            mx = ox;
            am = oi;
        }
        mn = fminf(mn, __shfl_xor(mn, o, 64));
    }
    if (lane == 0) {
        sh.red_max[w] = mx;
        sh.red_arg[w] = am;
        sh.red_min[w] = mn;
    }
    if (t == 0) {
        sh.pick = -1;
        sh.cut_bits = 0;
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < kSfWaves; ++v) {
        const float ox = sh.red_max[v];
        const int oi = sh.red_arg[v];
        if (ox > mx || (ox == mx && oi < am)) {
            mx = ox;
            am = oi;
        }
        mn = fminf(mn, sh.red_min[v]);
    }
    if (am < 0 || am >= V) am = 0;  // a row of NaNs
    r.mx = mx;
    r.c = T > 0.f ? fminf(1.44269504f / T, 3.0e38f) : 0.f;  // finite: 0 * c stays 0 for the maximum

    if (T == 0.f) {  // greedy row: the coin is drawn and dropped
        if (t == 0) {
            state[b] = st;
            next[b] = am;
            if (tokens) tokens[b] = am;
            if (pos) pos[b] += 1;
            if (n_kept) n_kept[b] = 1;
            if (cut_out) cut_out[b] = r.lg[am];
        }
        return;
    }

    // the cut: (cut key, n kept, ties kept at the cut)
    const bool haveK = k > 0 && k < V, haveP = P < 1.f;
    unsigned Kk = 0, tieK = 0, c_gt = 0, bin = 0;
    u64 m_gt = 0, target = 0;
    if (haveK) {
        Kk = sf_descend<false>(sh, r, false, 0u, 0u, (unsigned)k, 1.f, c_gt, m_gt, bin, target);
        tieK = (unsigned)k - c_gt;
    }
    float cutv;
    unsigned ties_kept, n;
    if (haveP) {
        const unsigned Kp = sf_descend<true>(sh, r, haveK, Kk, tieK, 0u, P, c_gt, m_gt, bin, target);
        cutv = sf_unkey(Kp);
        u64 wk = r.w(cutv);
        if (wk < 1) wk = 1;
        u64 j = target > m_gt ? (target - m_gt + wk - 1) / wk : 1;
        j = j < 1 ? 1 : j > bin ? bin : j;
        if (j < 1) j = 1;
        ties_kept = (unsigned)j;
        n = c_gt + ties_kept;
    } else if (haveK) {
        cutv = sf_unkey(Kk);
        ties_kept = tieK;
        n = (unsigned)k;
    } else {
        cutv = mn + 0.f;
        ties_kept = (unsigned)V;
        n = (unsigned)V;
    }
    const u64 wcut = r.w(cutv);

    // draw, stage 1: ties and mass above the cut of every part, in index order:
    // part 0 the head scalars, part 1 + w the float4s of wave w, last the tail
    const int Q = (r.nq + kSfWaves - 1) / kSfWaves;
    const int qlo = min(r.nq, w * Q), qhi = min(r.nq, qlo + Q);
    {
        unsigned ties = 0;
        u64 mass = 0;
        const float4* q4 = r.q4();
        for (int q0 = qlo; q0 < qhi; q0 += 64 * kSfLoads) {
            float4 v4[kSfLoads];
            sf_load(q4, q0 + lane, 64, qhi, v4);
#pragma unroll
            for (int u = 0; u < kSfLoads; ++u) {
                if (q0 + lane + 64 * u < qhi) {
                    const float4 v = v4[u];
                    const float x[4] = {v.x + 0.f, v.y + 0.f, v.z + 0.f, v.w + 0.f};
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (x[c] > cutv) mass += r.w(x[c]);
                        ties += x[c] == cutv;
                    }
                }
            }
        }
        ties = wave_sum_u32(ties);
        mass = wave_sum_u64(mass);
        if (lane == 0) {
            sh.seg_ties[1 + w] = ties;
            sh.seg_mass[1 + w] = mass;
        }
        if (t == 0) {
            for (int s = 0; s < 2; ++s) {
                const int lo = s ? r.tail0 : 0, hi = s ? V : r.head;
                unsigned tc = 0;
                u64 mc = 0;
                for (int i = lo; i < hi; ++i) {
                    const float x = r.lg[i] + 0.f;
                    if (x > cutv) mc += r.w(x);
                    tc += x == cutv;
                }
                sh.seg_ties[s ? kSfSegs - 1 : 0] = tc;
                sh.seg_mass[s ? kSfSegs - 1 : 0] = mc;
            }
        }
    }
    __syncthreads();
    // every thread: the kept total, the coin's threshold, and which part holds
    // the crossing and the last kept tie
    unsigned total_ties = 0;
    for (int s = 0; s < kSfSegs; ++s) total_ties += sh.seg_ties[s];
    const unsigned jj = min(ties_kept, total_ties);
    u64 S = 0;
    {
        unsigned tb = 0;
        for (int s = 0; s < kSfSegs; ++s) {
            const unsigned ts = sh.seg_ties[s];
            const unsigned kt = tb >= jj ? 0u : min(ts, jj - tb);
            S += sh.seg_mass[s] + (u64)kt * wcut;
            tb += ts;
        }
    }
    // running / S > u  <=>  running > floor(S * coin / 2^24)
    const u64 thr = (__umul64hi(S, coin) << 40) | ((S * coin) >> 24);
    const bool want_bits = cut_out && cutv == 0.f;  // the only value with two encodings
    int cross_seg = -1, tie_seg = -1;
    unsigned my_tb = 0;
    u64 my_mb = 0;
    {
        unsigned tb = 0;
        u64 mb = 0;
        for (int s = 0; s < kSfSegs; ++s) {
            const unsigned ts = sh.seg_ties[s];
            const unsigned kt = tb >= jj ? 0u : min(ts, jj - tb);
            const u64 ms = sh.seg_mass[s] + (u64)kt * wcut;
            if (cross_seg < 0 && mb + ms > thr) cross_seg = s;
            if (jj > 0 && tb <= jj - 1 && jj - 1 < tb + ts) tie_seg = s;
            if (s == 1 + w) {
                my_tb = tb;
                my_mb = mb;
            }
            tb += ts;
            mb += ms;
        }
    }
    // stage 2: scan the parts that matter in index order
    const int myseg = 1 + w;
    if (myseg == cross_seg || (want_bits && myseg == tie_seg)) {
        unsigned tb = my_tb;
        u64 mb = my_mb;
        const float4* q4 = r.q4();
        for (int qq = qlo; qq < qhi; qq += 64 * kSfLoads) {
          float4 v4[kSfLoads];
          sf_load(q4, qq + lane, 64, qhi, v4);
#pragma unroll
          for (int u = 0; u < kSfLoads; ++u) {  // in index order
            const int q0 = qq + 64 * u;
            if (q0 >= qhi) break;  // wave-uniform
            const int q = q0 + lane;
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            unsigned raw[4] = {0u, 0u, 0u, 0u};
            const bool ok = q < qhi;
            if (ok) {
                const float4 v = v4[u];
                raw[0] = __float_as_uint(v.x), raw[1] = __float_as_uint(v.y);
                raw[2] = __float_as_uint(v.z), raw[3] = __float_as_uint(v.w);
                x[0] = v.x + 0.f, x[1] = v.y + 0.f, x[2] = v.z + 0.f, x[3] = v.w + 0.f;
            }
            unsigned tc = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) tc += ok && x[c] == cutv;
            unsigned ti = tc;  // inclusive scan of the tie counts
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned u = __shfl_up(ti, o, 64);
                if (lane >= o) ti += u;
            }
            unsigned rank = tb + ti - tc;  // ties before this lane's first element
            u64 mw[4], ml = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                mw[c] = 0;
                if (ok && x[c] > cutv) mw[c] = r.w(x[c]);
                if (ok && x[c] == cutv) {
                    if (rank < jj) mw[c] = wcut;
                    if (want_bits && rank == jj - 1) sh.cut_bits = raw[c];
                    ++rank;
                }
                ml += mw[c];
            }
            u64 mi = ml;  // inclusive scan of the kept mass
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 u = __shfl_up(mi, o, 64);
                if (lane >= o) mi += u;
            }
            u64 run = mb + mi - ml;
            if (run <= thr && run + ml > thr) {  // the crossing is in this lane: one lane at most
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (run <= thr && run + mw[c] > thr) sh.pick = r.head + 4 * q + c;
                    run += mw[c];
                }
            }
            tb += __shfl(ti, 63, 64);
            mb += __shfl(mi, 63, 64);
          }
        }
    }
    if (t == 0) {  // the head and tail scalars
        for (int s = 0; s < 2; ++s) {
            const int seg = s ? kSfSegs - 1 : 0;
            if (seg != cross_seg && !(want_bits && seg == tie_seg)) continue;
            unsigned tb = 0;
            u64 mb = 0;
            for (int q = 0; q < seg; ++q) {
                const unsigned ts = sh.seg_ties[q];
                const unsigned kt = tb >= jj ? 0u : min(ts, jj - tb);
                mb += sh.seg_mass[q] + (u64)kt * wcut;
                tb += ts;
            }
            const int lo = s ? r.tail0 : 0, hi = s ? V : r.head;
            for (int i = lo; i < hi; ++i) {
                const float xr = r.lg[i], x = xr + 0.f;
                u64 mw = 0;
                if (x > cutv) mw = r.w(x);
                if (x == cutv) {
                    if (tb < jj) mw = wcut;
                    if (want_bits && tb == jj - 1) sh.cut_bits = __float_as_uint(xr);
                    ++tb;
                }
                if (mb <= thr && mb + mw > thr) sh.pick = i;
                mb += mw;
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        // S > 0 and coin < 2^24, so the integer cdf always passes the coin; the
        // row maximum (always kept) stands in if a NaN row defeated the sums
        int pick = sh.pick;
        if (pick < 0 || pick >= V) pick = am;
        state[b] = st;
        next[b] = pick;
        if (tokens) tokens[b] = pick;
        if (pos) pos[b] += 1;
        if (n_kept) n_kept[b] = (int)n;
        if (cut_out) cut_out[b] = want_bits ? __uint_as_float(sh.cut_bits) : cutv;
    }
}
}  // namespace

int hpa_sample_filtered(const float* logits, int B, int V, const float* temperature, const int* top_k,
                        const float* top_p, unsigned long long* state, int* next, int* tokens, int* pos,
                        const int* active, int* n_kept, float* cut) {
    HPA_REQUIRE(logits && temperature && top_k && top_p && state && next && B > 0 && V > 0,
                "sample_filtered: bad arguments");
    int lg = 0;  // ceil(log2 V)
    while ((1ll << lg) < (long long)V) ++lg;
    const int shift = 62 - lg < 44 ? 62 - lg : 44;  // V masses of at most 2^shift sum below 2^62
    sample_filtered_kernel<<<B, kSfThreads, 0, hpa_stream()>>>(logits, V, temperature, top_k, top_p, state, next,
                                                               tokens, pos, active, n_kept, cut, shift);
    HPA_LAUNCH_CHECK();
    return 0;
}
