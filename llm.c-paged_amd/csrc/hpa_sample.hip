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
//
// Speculative sampling (gpt2_decode_verify_sampled) is built from the same
// passes, factored into device functions (sf_filter, sf_parts, sf_total,
// sf_id_mass): hpa_sample_filtered_prob runs the filter for many rows and
// reports the kept total and one id's mass, without coin or draw;
// hpa_sample_filtered_ex is the sampler with one id taken out of the kept set
// before the draw (hpa_sample_filtered: the instantiation without it);
// hpa_spec_accept walks a sequence's drafted rows, one coin each, and accepts
// while  w_target * 2^24 > w_total * j.
//
// Sampled tree speculation (gpt2_decode_verify_tree_sampled) adds the list
// forms: hpa_sample_filtered_prob_multi (up to 7 ids per row in one pass over
// the row: sf_parts keeps one tie-rank counter per id), hpa_sample_filtered_exn
// (the sampler with a list of ids taken out, a third instantiation) and
// hpa_spec_tree_accept (the multi-draft walk: the children of a node in turn,
// each against what the siblings rejected before it left of the node's total).
#include <limits.h>
#include <math.h>

#include "hpa_internal.h"

namespace {
typedef unsigned long long u64;
constexpr int kSfThreads = 1024;
constexpr int kSfWaves = kSfThreads / 64;
constexpr int kSfSegs = kSfWaves + 2;  // head scalars, one part per wave, tail scalars
constexpr int kSfMulti = HPA_VERIFY_MAX_ROWS - 1;  // ids a row can single out in the list forms

struct SfShared {
    unsigned cnt[256];
    u64 mass[256];
    float red_max[kSfWaves], red_min[kSfWaves];
    int red_arg[kSfWaves];
    unsigned seg_ties[kSfSegs];
    unsigned seg_tlt[kSfSegs];  // ties below the singled-out id (sf_parts<1>)
    u64 seg_mass[kSfSegs];
    unsigned digit, bin_count, c_above;
    u64 m_above, target;
    int pick;
    unsigned cut_bits;
};
// the list forms' tie ranks: one row of parts per singled-out id
template <int N>
struct SfTies {
    unsigned v[N][kSfSegs];
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

__device__ __forceinline__ void sf_row_init(SfRow& r, const float* lg, int V, int shift) {
    r.lg = lg;
    r.V = V;
    r.head = min(V, (int)((4u - (unsigned)(((size_t)r.lg >> 2) & 3u)) & 3u));
    r.nq = (V - r.head) >> 2;
    r.tail0 = r.head + 4 * r.nq;
    r.scale = (float)(1ull << shift);
}

// per-row parameters, sanitised so that nothing below can leave the row
__device__ __forceinline__ void sf_settings(float& T, int& k, float& P) {
    if (!(T >= 0.f) || isinf(T)) T = 1.f;
    if (k < 0) k = 0;
    if (!(P > 0.f && P <= 1.f)) P = 1.f;
}

// The filter of one row, every thread of the workgroup: pass 1 and the radix
// descents.  Sets r.mx and r.c; am: the lowest-index argmax.  Returns false
// for a greedy row (T == 0: nothing after pass 1); else the cut: its value,
// the ties kept at it and the kept count n.  Resets sh.pick and sh.cut_bits.
__device__ __forceinline__ bool sf_filter(SfShared& sh, SfRow& r, float T, int k, float P, int& am_out, float& cutv,
                                          unsigned& ties_kept, unsigned& n) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int V = r.V;
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
    am_out = am;
    if (T == 0.f) return false;

    // the cut: (cut key, n kept, ties kept at the cut)
    const bool haveK = k > 0 && k < V, haveP = P < 1.f;
    unsigned Kk = 0, tieK = 0, c_gt = 0, bin = 0;
    u64 m_gt = 0, target = 0;
    if (haveK) {
        Kk = sf_descend<false>(sh, r, false, 0u, 0u, (unsigned)k, 1.f, c_gt, m_gt, bin, target);
        tieK = (unsigned)k - c_gt;
    }
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
    return true;
}

// Ties and mass above the cut of every part of the row, in index order: part 0
// the head scalars, part 1 + w the float4s of wave w, last the tail.  NE > 0:
// also, per singled-out id e[i], the ties at an index below it (its tie rank),
// into seg_tlt[i]; one pass over the row whatever NE is (e: NE ids, at least
// one slot).  The caller synchronises before it reads sh.seg_* and seg_tlt.
template <int NE>
__device__ __forceinline__ void sf_parts(SfShared& sh, const SfRow& r, float cutv, const int (&e)[NE > 0 ? NE : 1],
                                         unsigned (*seg_tlt)[kSfSegs]) {
    constexpr int NT = NE > 0 ? NE : 1;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int Q = (r.nq + kSfWaves - 1) / kSfWaves;
    const int qlo = min(r.nq, w * Q), qhi = min(r.nq, qlo + Q);
    unsigned ties = 0, tlt[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) tlt[i] = 0;
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
                    if (NE == 1) tlt[0] += x[c] == cutv && r.head + 4 * (q0 + lane + 64 * u) + c < e[0];
                    if (NE > 1 && x[c] == cutv) {  // ties are few: the NE compares stay off the common path
#pragma unroll
                        for (int i = 0; i < NT; ++i) tlt[i] += r.head + 4 * (q0 + lane + 64 * u) + c < e[i];
                    }
                }
            }
        }
    }
    ties = wave_sum_u32(ties);
    mass = wave_sum_u64(mass);
    if (NE > 0) {
#pragma unroll
        for (int i = 0; i < NT; ++i) tlt[i] = wave_sum_u32(tlt[i]);
    }
    if (lane == 0) {
        sh.seg_ties[1 + w] = ties;
        sh.seg_mass[1 + w] = mass;
        if (NE > 0) {
#pragma unroll
            for (int i = 0; i < NT; ++i) seg_tlt[i][1 + w] = tlt[i];
        }
    }
    if (t == 0) {
        for (int s = 0; s < 2; ++s) {
            const int lo = s ? r.tail0 : 0, hi = s ? r.V : r.head;
            unsigned tc = 0, tl[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) tl[i] = 0;
            u64 mc = 0;
            for (int i = lo; i < hi; ++i) {
                const float x = r.lg[i] + 0.f;
                if (x > cutv) mc += r.w(x);
                tc += x == cutv;
                if (NE > 0) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) tl[j] += x == cutv && i < e[j];
                }
            }
            sh.seg_ties[s ? kSfSegs - 1 : 0] = tc;
            sh.seg_mass[s ? kSfSegs - 1 : 0] = mc;
            if (NE > 0) {
#pragma unroll
                for (int j = 0; j < NT; ++j) seg_tlt[j][s ? kSfSegs - 1 : 0] = tl[j];
            }
        }
    }
}

// the kept total S and the number jj of ties kept, from the parts (every thread)
__device__ __forceinline__ u64 sf_total(const SfShared& sh, unsigned ties_kept, u64 wcut, unsigned& jj) {
    unsigned total_ties = 0;
    for (int s = 0; s < kSfSegs; ++s) total_ties += sh.seg_ties[s];
    jj = min(ties_kept, total_ties);
    u64 S = 0;
    unsigned tb = 0;
    for (int s = 0; s < kSfSegs; ++s) {
        const unsigned ts = sh.seg_ties[s];
        const unsigned kt = tb >= jj ? 0u : min(ts, jj - tb);
        S += sh.seg_mass[s] + (u64)kt * wcut;
        tb += ts;
    }
    return S;
}

// the mass id e (in [0, V)) has in the draw, after sf_parts singled it out with
// its tie ranks in seg_tlt: above the cut its own, at the cut wcut if its tie
// rank is kept, else 0
__device__ __forceinline__ u64 sf_id_mass(const unsigned* seg_tlt, const SfRow& r, float cutv, u64 wcut, unsigned jj,
                                          int e) {
    unsigned tlt = 0;
    for (int s = 0; s < kSfSegs; ++s) tlt += seg_tlt[s];
    const float xe = r.lg[e] + 0.f;
    return xe > cutv ? r.w(xe) : (xe == cutv && tlt < jj) ? wcut : 0;
}

// the part that holds index e
__device__ __forceinline__ int sf_seg_of(const SfRow& r, int e) {
    if (e < r.head) return 0;
    if (e >= r.tail0) return kSfSegs - 1;
    const int Q = (r.nq + kSfWaves - 1) / kSfWaves;
    return 1 + ((e - r.head) >> 2) / Q;
}

// EX = 1: exclude[b] (-1: none) is taken out of the kept set before the draw;
// EX = 2: the first n_exclude[b] ids of exclude[b][kSfMulti] are
template <int EX>
__global__ __launch_bounds__(kSfThreads) void sample_filtered_kernel(
    const float* __restrict__ logits, int V, const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, unsigned long long* __restrict__ state, int* __restrict__ next,
    int* __restrict__ tokens, int* __restrict__ pos, const int* __restrict__ active, int* __restrict__ n_kept,
    float* __restrict__ cut_out, const int* __restrict__ exclude, const int* __restrict__ n_exclude, int shift) {
    constexpr int NX = EX == 2 ? kSfMulti : 1;
    __shared__ SfShared sh;
    __shared__ SfTies<NX> tie_sh;  // EX < 2: sh.seg_tlt serves, this one is never touched
    unsigned (*seg_tlt)[kSfSegs] = EX == 2 ? tie_sh.v : &sh.seg_tlt;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (active && active[b] <= 0) return;  // row left as it is (its RNG state too)
    SfRow r;
    sf_row_init(r, logits + (size_t)b * V, V, shift);
    float T = temperature[b];
    int k = top_k[b];
    float P = top_p[b];
    sf_settings(T, k, P);
    unsigned long long st = state[b];
    const u64 coin = hpa::xorshift_u32(st) >> 8;  // u = coin / 2^24
    int ex[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) ex[i] = -1;
    if (EX == 1) {
        ex[0] = exclude[b];
        if (ex[0] < 0 || ex[0] >= V) ex[0] = -1;
    }
    if (EX == 2) {  // ids outside [0, V) and repeats remove nothing
        const int nx = min(max(n_exclude[b], 0), NX);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            int id = i < nx ? exclude[b * NX + i] : -1;
            if (id < 0 || id >= V) id = -1;
#pragma unroll
            for (int j = 0; j < i; ++j)
                if (ex[j] == id) id = -1;
            ex[i] = id;
        }
    }

    int am;
    float cutv;
    unsigned ties_kept, n;
    if (!sf_filter(sh, r, T, k, P, am, cutv, ties_kept, n)) {  // greedy row: the coin is drawn and dropped
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
    const u64 wcut = r.w(cutv);

    // draw, stage 1: the parts
    const int Q = (r.nq + kSfWaves - 1) / kSfWaves;
    const int qlo = min(r.nq, w * Q), qhi = min(r.nq, qlo + Q);
    sf_parts<EX == 2 ? NX : EX>(sh, r, cutv, ex, seg_tlt);
    __syncthreads();
    // every thread: the kept total, the coin's threshold, and which part holds
    // the crossing and the last kept tie
    unsigned jj;
    u64 S = sf_total(sh, ties_kept, wcut, jj);
    // an excluded id's mass leaves its part and the total; exclusions that
    // would leave nothing are dropped, all of them, and one that removes nothing is
    u64 wex[NX];
    int exseg[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        wex[i] = 0;
        exseg[i] = -1;
    }
    if (EX) {
        u64 wsum = 0;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            if (ex[i] >= 0) wex[i] = sf_id_mass(seg_tlt[i], r, cutv, wcut, jj, ex[i]);
            wsum += wex[i];
        }
        if (wsum >= S) {
            wsum = 0;
#pragma unroll
            for (int i = 0; i < NX; ++i) wex[i] = 0;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            if (wex[i] == 0) ex[i] = -1;
            else exseg[i] = sf_seg_of(r, ex[i]);
        }
        S -= wsum;
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
            u64 ms = sh.seg_mass[s] + (u64)kt * wcut;
            if (EX) {
#pragma unroll
                for (int i = 0; i < NX; ++i)
                    if (s == exseg[i]) ms -= wex[i];
            }
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
                if (EX) {
#pragma unroll
                    for (int i = 0; i < NX; ++i)
                        if (r.head + 4 * q + c == ex[i]) mw[c] = 0;
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
                if (EX) {
#pragma unroll
                    for (int i = 0; i < NX; ++i)
                        if (q == exseg[i]) mb -= wex[i];
                }
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
                if (EX) {
#pragma unroll
                    for (int j = 0; j < NX; ++j)
                        if (i == ex[j]) mw = 0;
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

// the raw bits of the last kept tie (rank jj - 1 in index order) into
// sh.cut_bits: the stage-2 tie scan without the draw (the caller synchronises)
__device__ __forceinline__ void sf_cut_bits(SfShared& sh, const SfRow& r, float cutv, unsigned jj) {
    if (jj == 0) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int tie_seg = -1;
    unsigned seg_tb = 0;
    {
        unsigned tb = 0;
        for (int s = 0; s < kSfSegs; ++s) {
            const unsigned ts = sh.seg_ties[s];
            if (tb <= jj - 1 && jj - 1 < tb + ts) {
                tie_seg = s;
                seg_tb = tb;
            }
            tb += ts;
        }
    }
    if (tie_seg == 1 + w) {
        const int Q = (r.nq + kSfWaves - 1) / kSfWaves;
        const int qlo = min(r.nq, w * Q), qhi = min(r.nq, qlo + Q);
        const float4* q4 = r.q4();
        unsigned tb = seg_tb;
        for (int q0 = qlo; q0 < qhi; q0 += 64) {  // wave-uniform, in index order
            const int q = q0 + lane;
            const bool ok = q < qhi;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) v = q4[q];
            const unsigned raw[4] = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z),
                                     __float_as_uint(v.w)};
            const float x[4] = {v.x + 0.f, v.y + 0.f, v.z + 0.f, v.w + 0.f};
            unsigned tc = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) tc += ok && x[c] == cutv;
            unsigned ti = tc;  // inclusive scan of the tie counts
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned u = __shfl_up(ti, o, 64);
                if (lane >= o) ti += u;
            }
            unsigned rank = tb + ti - tc;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (ok && x[c] == cutv) {
                    if (rank == jj - 1) sh.cut_bits = raw[c];
                    ++rank;
                }
            }
            tb += __shfl(ti, 63, 64);
        }
    }
    if (t == 0 && (tie_seg == 0 || tie_seg == kSfSegs - 1)) {
        const int lo = tie_seg ? r.tail0 : 0, hi = tie_seg ? r.V : r.head;
        unsigned tb = seg_tb;
        for (int i = lo; i < hi; ++i) {
            const float xr = r.lg[i];
            if (xr + 0.f == cutv) {
                if (tb == jj - 1) sh.cut_bits = __float_as_uint(xr);
                ++tb;
            }
        }
    }
}

// The filter of R rows and the mass of one id per row: sample_filtered_kernel
// up to the kept total, without coin, state or draw.
__global__ __launch_bounds__(kSfThreads) void sample_filtered_prob_kernel(
    const float* __restrict__ logits, int V, const int* __restrict__ seq, const float* __restrict__ temperature,
    const int* __restrict__ top_k, const float* __restrict__ top_p, const int* __restrict__ target,
    int* __restrict__ n_kept, float* __restrict__ cut_out, unsigned long long* __restrict__ w_target,
    unsigned long long* __restrict__ w_total, int shift) {
    __shared__ SfShared sh;
    const int row = blockIdx.x, t = threadIdx.x;
    const int b = seq ? seq[row] : row;
    SfRow r;
    sf_row_init(r, logits + (size_t)row * V, V, shift);
    float T = temperature[b];
    int k = top_k[b];
    float P = top_p[b];
    sf_settings(T, k, P);
    int d = target[row];
    if (d < 0 || d >= V) d = -1;

    int am;
    float cutv;
    unsigned ties_kept, n;
    if (!sf_filter(sh, r, T, k, P, am, cutv, ties_kept, n)) {  // greedy row: a point mass at the argmax
        if (t == 0) {
            if (n_kept) n_kept[row] = 1;
            if (cut_out) cut_out[row] = r.lg[am];
            w_target[row] = d == am ? 1ull : 0ull;
            w_total[row] = 1ull;
        }
        return;
    }
    const u64 wcut = r.w(cutv);
    const int ds[1] = {d};
    sf_parts<1>(sh, r, cutv, ds, &sh.seg_tlt);
    __syncthreads();
    unsigned jj;
    const u64 S = sf_total(sh, ties_kept, wcut, jj);
    const bool want_bits = cut_out && cutv == 0.f;  // the only value with two encodings
    if (want_bits) {
        sf_cut_bits(sh, r, cutv, jj);
        __syncthreads();
    }
    if (t == 0) {
        if (n_kept) n_kept[row] = (int)n;
        if (cut_out) cut_out[row] = want_bits ? __uint_as_float(sh.cut_bits) : cutv;
        w_target[row] = d >= 0 ? sf_id_mass(sh.seg_tlt, r, cutv, wcut, jj, d) : 0ull;
        w_total[row] = S;
    }
}

// sample_filtered_prob_kernel for a list of ids per row: the row is read once
// (one tie-rank counter per id in sf_parts); the total, n_kept and the cut are
// computed once.  Entry i's mass and the row's total go to w_target / w_total
// [dst[row][i]]: the caller's packing (by draft, in the tree pass).
__global__ __launch_bounds__(kSfThreads) void sample_filtered_prob_multi_kernel(
    const float* __restrict__ logits, int V, const int* __restrict__ seq, const float* __restrict__ temperature,
    const int* __restrict__ top_k, const float* __restrict__ top_p, const int* __restrict__ targets,
    const int* __restrict__ n_targets, const int* __restrict__ dst, int* __restrict__ n_kept,
    float* __restrict__ cut_out, unsigned long long* __restrict__ w_target, unsigned long long* __restrict__ w_total,
    int shift) {
    __shared__ SfShared sh;
    __shared__ SfTies<kSfMulti> tie_sh;
    const int row = blockIdx.x, t = threadIdx.x;
    const int b = seq ? seq[row] : row;
    SfRow r;
    sf_row_init(r, logits + (size_t)row * V, V, shift);
    float T = temperature[b];
    int k = top_k[b];
    float P = top_p[b];
    sf_settings(T, k, P);
    const int m = min(max(n_targets[row], 0), kSfMulti);
    int d[kSfMulti], o[kSfMulti];
#pragma unroll
    for (int i = 0; i < kSfMulti; ++i) {
        d[i] = i < m ? targets[row * kSfMulti + i] : -1;
        if (d[i] < 0 || d[i] >= V) d[i] = -1;
        o[i] = i < m ? dst[row * kSfMulti + i] : -1;
    }

    int am;
    float cutv;
    unsigned ties_kept, n;
    if (!sf_filter(sh, r, T, k, P, am, cutv, ties_kept, n)) {  // greedy row: a point mass at the argmax
        if (t == 0) {
            if (n_kept) n_kept[row] = 1;
            if (cut_out) cut_out[row] = r.lg[am];
#pragma unroll
            for (int i = 0; i < kSfMulti; ++i)
                if (o[i] >= 0) {
                    w_target[o[i]] = d[i] == am ? 1ull : 0ull;
                    w_total[o[i]] = 1ull;
                }
        }
        return;
    }
    const u64 wcut = r.w(cutv);
    sf_parts<kSfMulti>(sh, r, cutv, d, tie_sh.v);
    __syncthreads();
    unsigned jj;
    const u64 S = sf_total(sh, ties_kept, wcut, jj);
    const bool want_bits = cut_out && cutv == 0.f;  // the only value with two encodings
    if (want_bits) {
        sf_cut_bits(sh, r, cutv, jj);
        __syncthreads();
    }
    if (t == 0) {
        if (n_kept) n_kept[row] = (int)n;
        if (cut_out) cut_out[row] = want_bits ? __uint_as_float(sh.cut_bits) : cutv;
#pragma unroll
        for (int i = 0; i < kSfMulti; ++i)
            if (o[i] >= 0) {
                w_target[o[i]] = d[i] >= 0 ? sf_id_mass(tie_sh.v[i], r, cutv, wcut, jj, d[i]) : 0ull;
                w_total[o[i]] = S;
            }
    }
}

// The accept walk of speculative sampling, one thread per sequence (plain
// integer arithmetic: the products are compared as 128-bit numbers).
__global__ __launch_bounds__(64) void spec_accept_kernel(
    const unsigned long long* __restrict__ w_target, const unsigned long long* __restrict__ w_total,
    const int* __restrict__ drafts, const int* __restrict__ draft0, const int* __restrict__ start,
    const int* __restrict__ row0, const int* __restrict__ len, int B, unsigned long long* __restrict__ state,
    int* __restrict__ n_accepted, int* __restrict__ cont_row, int* __restrict__ exclude, int* __restrict__ pos) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int n = len[b];
    if (n <= 0) {  // untouched: state and position left as they are
        n_accepted[b] = -1;
        cont_row[b] = -1;
        exclude[b] = -1;
        return;
    }
    const int d0 = draft0[b];
    unsigned long long st = state[b];
    int a = 0, rejected = -1;
    while (a + 1 < n) {
        const u64 j = hpa::xorshift_u32(st) >> 8;  // u = j / 2^24
        const u64 wt = w_target[d0 + a], ws = w_total[d0 + a];
        // wt * 2^24 > ws * j
        const u64 lhi = wt >> 40, llo = wt << 24;
        const u64 rhi = __umul64hi(ws, j), rlo = ws * j;
        if (!(lhi > rhi || (lhi == rhi && llo > rlo))) {
            rejected = drafts[d0 + a];
            break;
        }
        ++a;
    }
    state[b] = st;
    n_accepted[b] = a;
    cont_row[b] = row0[b] + a;
    exclude[b] = rejected;
    pos[b] = start[b] + a;
}

// The accept walk of sampled tree speculation, one thread per sequence: the
// children of the current node in ascending node index, one coin each, against
// what is left of the node's total once the children rejected before are
// taken out.  w_target / w_total are packed by draft (draft j = node j + 1):
// the draft's mass at its parent's row and that row's total.  A parent
// outside [0, j] is clamped as in verify_tree_rows_kernel: an accepted child
// has a larger index than its parent, so the walk takes at most n - 1 steps
// whatever the table holds.
__global__ __launch_bounds__(64) void spec_tree_accept_kernel(
    const unsigned long long* __restrict__ w_target, const unsigned long long* __restrict__ w_total,
    const int* __restrict__ drafts, const int* __restrict__ parents, const int* __restrict__ doffs,
    const int* __restrict__ start, const int* __restrict__ row0, const int* __restrict__ len, int B,
    unsigned long long* __restrict__ state, int* __restrict__ n_accepted, int* __restrict__ path,
    int* __restrict__ cont_row, int* __restrict__ exclude, int* __restrict__ n_exclude, int* __restrict__ pos) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int* excl = exclude + (size_t)b * kSfMulti;
    const int n = min(len[b], HPA_VERIFY_MAX_ROWS);
    if (n <= 0) {  // untouched: state and position left as they are
        n_accepted[b] = -1;
        cont_row[b] = -1;
        n_exclude[b] = 0;
        for (int i = 0; i < kSfMulti; ++i) excl[i] = -1;
        return;
    }
    const int doff = doffs[b];
    unsigned long long st = state[b];
    int cur = 0, a = 0, nrej = 0;
    for (;;) {
        nrej = 0;  // the rejected children of this node, in child order
        u64 rem = 0;
        int next = -1;
        for (int c = cur + 1; c < n; ++c) {
            if (min(max(parents[doff + c - 1], 0), c - 1) != cur) continue;
            if (nrej == 0) rem = w_total[doff + c - 1];  // the first child: the node's kept total
            const u64 j = hpa::xorshift_u32(st) >> 8;  // u = j / 2^24
            const u64 wt = w_target[doff + c - 1];
            // wt * 2^24 > rem * j
            const u64 lhi = wt >> 40, llo = wt << 24;
            const u64 rhi = __umul64hi(rem, j), rlo = rem * j;
            if (lhi > rhi || (lhi == rhi && llo > rlo)) {
                next = c;
                break;
            }
            rem -= wt < rem ? wt : rem;  // a rejected child has wt < rem
            excl[nrej++] = drafts[doff + c - 1];
        }
        if (next < 0) break;
        path[b * HPA_VERIFY_MAX_ROWS + a++] = next;  // next > cur: at most n - 1 steps
        cur = next;
    }
    for (int i = nrej; i < kSfMulti; ++i) excl[i] = -1;
    state[b] = st;
    n_accepted[b] = a;
    cont_row[b] = row0[b] + cur;
    n_exclude[b] = nrej;
    pos[b] = start[b] + a;
}

// V masses of at most 2^shift sum below 2^62
int sf_shift(int V) {
    int lg = 0;  // ceil(log2 V)
    while ((1ll << lg) < (long long)V) ++lg;
    return 62 - lg < 44 ? 62 - lg : 44;
}
}  // namespace

int hpa_sample_filtered_ex(const float* logits, int B, int V, const float* temperature, const int* top_k,
                           const float* top_p, unsigned long long* state, int* next, int* tokens, int* pos,
                           const int* active, int* n_kept, float* cut, const int* exclude) {
    HPA_REQUIRE(logits && temperature && top_k && top_p && state && next && B > 0 && V > 0,
                "sample_filtered: bad arguments");
    const int shift = sf_shift(V);
    if (exclude)
        sample_filtered_kernel<1><<<B, kSfThreads, 0, hpa_stream()>>>(
            logits, V, temperature, top_k, top_p, state, next, tokens, pos, active, n_kept, cut, exclude, nullptr, shift);
    else
        sample_filtered_kernel<0><<<B, kSfThreads, 0, hpa_stream()>>>(
            logits, V, temperature, top_k, top_p, state, next, tokens, pos, active, n_kept, cut, nullptr, nullptr, shift);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_sample_filtered_exn(const float* logits, int B, int V, const float* temperature, const int* top_k,
                            const float* top_p, unsigned long long* state, int* next, int* tokens, int* pos,
                            const int* active, int* n_kept, float* cut, const int* exclude, const int* n_exclude) {
    HPA_REQUIRE(logits && temperature && top_k && top_p && state && next && exclude && n_exclude && B > 0 && V > 0,
                "sample_filtered_exn: bad arguments");
    sample_filtered_kernel<2><<<B, kSfThreads, 0, hpa_stream()>>>(logits, V, temperature, top_k, top_p, state, next,
                                                                  tokens, pos, active, n_kept, cut, exclude, n_exclude,
                                                                  sf_shift(V));
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_sample_filtered(const float* logits, int B, int V, const float* temperature, const int* top_k,
                        const float* top_p, unsigned long long* state, int* next, int* tokens, int* pos,
                        const int* active, int* n_kept, float* cut) {
    return hpa_sample_filtered_ex(logits, B, V, temperature, top_k, top_p, state, next, tokens, pos, active, n_kept,
                                  cut, NULL);
}

int hpa_sample_filtered_prob(const float* logits, int R, int V, const int* seq, const float* temperature,
                             const int* top_k, const float* top_p, const int* target, int* n_kept, float* cut,
                             unsigned long long* w_target, unsigned long long* w_total) {
    HPA_REQUIRE(logits && temperature && top_k && top_p && target && w_target && w_total && R > 0 && V > 0,
                "sample_filtered_prob: bad arguments");
    sample_filtered_prob_kernel<<<R, kSfThreads, 0, hpa_stream()>>>(logits, V, seq, temperature, top_k, top_p, target,
                                                                    n_kept, cut, w_target, w_total, sf_shift(V));
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_spec_accept(const unsigned long long* w_target, const unsigned long long* w_total, const int* drafts,
                    const int* draft0, const int* start, const int* row0, const int* len, int B,
                    unsigned long long* state, int* n_accepted, int* cont_row, int* exclude, int* pos) {
    HPA_REQUIRE(w_target && w_total && drafts && draft0 && start && row0 && len && state && n_accepted && cont_row &&
                    exclude && pos && B > 0,
                "spec accept: bad arguments");
    spec_accept_kernel<<<(unsigned)((B + 63) / 64), 64, 0, hpa_stream()>>>(
        w_target, w_total, drafts, draft0, start, row0, len, B, state, n_accepted, cont_row, exclude, pos);
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_sample_filtered_prob_multi(const float* logits, int R, int V, const int* seq, const float* temperature,
                                   const int* top_k, const float* top_p, const int* targets, const int* n_targets,
                                   const int* dst, int* n_kept, float* cut, unsigned long long* w_target,
                                   unsigned long long* w_total) {
    HPA_REQUIRE(logits && temperature && top_k && top_p && targets && n_targets && dst && w_target && w_total && R > 0 &&
                    V > 0,
                "sample_filtered_prob_multi: bad arguments");
    sample_filtered_prob_multi_kernel<<<R, kSfThreads, 0, hpa_stream()>>>(
        logits, V, seq, temperature, top_k, top_p, targets, n_targets, dst, n_kept, cut, w_target, w_total, sf_shift(V));
    HPA_LAUNCH_CHECK();
    return 0;
}

int hpa_spec_tree_accept(const unsigned long long* w_target, const unsigned long long* w_total, const int* drafts,
                         const int* parents, const int* draft0, const int* start, const int* row0, const int* len, int B,
                         unsigned long long* state, int* n_accepted, int* path, int* cont_row, int* exclude,
                         int* n_exclude, int* pos) {
    HPA_REQUIRE(w_target && w_total && drafts && parents && draft0 && start && row0 && len && state && n_accepted &&
                    path && cont_row && exclude && n_exclude && pos && B > 0,
                "spec tree accept: bad arguments");
    spec_tree_accept_kernel<<<(unsigned)((B + 63) / 64), 64, 0, hpa_stream()>>>(
        w_target, w_total, drafts, parents, draft0, start, row0, len, B, state, n_accepted, path, cont_row, exclude,
        n_exclude, pos);
    HPA_LAUNCH_CHECK();
    return 0;
}
