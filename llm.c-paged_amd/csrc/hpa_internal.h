// hpa_internal.h -- shared by the HIP translation units of libpaged_hip.so.
// gfx950 (CDNA4) only: wave64, fp32 MFMA, no CUDA compatibility layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "hip_paged_attn.h"

// Returns a nonzero status after reporting; exits when HPA_FATAL=1
// (cudaCheck convention, reference train_gpt2.cu:27-34).
int hpa_fail(const char* file, int line, const char* what);
hipStream_t hpa_stream();

#define HPA_CHECK(call)                                                          \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return hpa_fail(__FILE__, __LINE__, hipGetErrorString(e_)); \
    } while (0)

#define HPA_REQUIRE(cond, msg)                                                   \
    do {                                                                         \
        if (!(cond)) return hpa_fail(__FILE__, __LINE__, msg);                   \
    } while (0)

// checks the launch that was just enqueued
#define HPA_LAUNCH_CHECK() HPA_CHECK(hipGetLastError())

namespace hpa {
constexpr int kWave = 64;

// CUs of the current device (0: no device), read once per process
int num_cus();

// blocks per CU of Kernel at `threads` per block (occupancy API), cached per kernel
template <auto Kernel>
int resident_blocks(int threads) {
    static int resident = -1;
    if (resident < 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kernel, threads, 0) != hipSuccess) nb = 0;
        resident = nb;
    }
    return resident;
}

// the launchers' template arguments from a pool: f(std::integral_constant<int, P>,
// std::bool_constant<BF>) with P the page size (8, 16, 32 or 64) and BF = bf16
// pool (fp32 and fp8 pools: false); any other page size fails with msg
template <typename F>
int with_page_dtype(const HpaKVPool* pool, const char* msg, F&& f) {
    auto by_dtype = [&](auto p) {
        return pool->dtype == HPA_BF16 ? f(p, std::true_type{}) : f(p, std::false_type{});
    };
    switch (pool->page_size) {
        case 8: return by_dtype(std::integral_constant<int, 8>{});
        case 16: return by_dtype(std::integral_constant<int, 16>{});
        case 32: return by_dtype(std::integral_constant<int, 32>{});
        case 64: return by_dtype(std::integral_constant<int, 64>{});
        default: return hpa_fail(__FILE__, __LINE__, msg);
    }
}

// 16-byte write-through (sc1) store / L1-bypassing (sc1) load at
// base + byte_off (base wave-uniform, byte_off per lane, 16-B aligned): the
// hand-off forms of MI355X_MICROARCH.md "Valid forms" row 1 at full width
// (4-byte sc1 stores are one fabric write each, several times slower per byte)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int kCpolSc1 = 16;  // gfx940+ cache policy: SC1
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void store_wt16(void* base, int byte_off, float4 v) {
    const u32x4 d = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(d, wt_rsrc(base), byte_off, 0, kCpolSc1);
}
__device__ __forceinline__ float4 load_wt16(const void* base, int byte_off) {
    const u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(wt_rsrc(base), byte_off, 0, kCpolSc1);
    return make_float4(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z), __uint_as_float(d.w));
}

// 4-byte forms (one float per lane; a wave's 64 consecutive floats are one
// 256-B write-through burst)
__device__ __forceinline__ void store_wt4(void* base, int byte_off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), wt_rsrc(base), byte_off, 0, kCpolSc1);
}
__device__ __forceinline__ float load_wt4(const void* base, int byte_off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wt_rsrc(base), byte_off, 0, kCpolSc1));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the reference's xorshift* generator (random_u32, paged_infer.c:826-830); the
// samplers' coin is (xorshift_u32(state) >> 8) / 16777216.0f (random_f32)
__device__ __forceinline__ unsigned int xorshift_u32(unsigned long long& s) {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return (unsigned int)((s * 0x2545F4914F6CDD1Dull) >> 32);
}

// "frag" layout of a [rows][K] fp32 matrix (rows padded to 16, K % 16 == 0),
// the operand layout of v_mfma_f32_16x16x4_f32 loaded 16 bytes per lane:
// element (m, k) sits at lane (m%16) + 16*((k%16)/4), float (k%4) of the
// 1 KiB fragment of (16-row block m/16, 16-deep k-step k/16); fragment
// (rb, kb) starts at ((rb * K/16 + kb) * 64) float4s.  A wave loads one
// fragment as one contiguous 1 KiB dwordx4 burst.  Used for streamed weights
// and for every activation that feeds a GEMM.
__device__ __host__ __forceinline__ size_t frag_index(int m, int k, int K) {
    return ((((size_t)(m >> 4) * (size_t)(K >> 4) + (size_t)(k >> 4)) * 64 +
             (size_t)((m & 15) + 16 * ((k >> 2) & 3)))
            << 2) +
           (size_t)(k & 3);
}

// fp32 -> bf16, round to nearest even (finite inputs; the KV pool's storage)
__device__ __host__ __forceinline__ unsigned short f32_to_bf16(float f) {
    unsigned int u;
    __builtin_memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// fp8 KV storage (HPA_FP8): OCP e4m3fn codes on gfx950's hardware converts.
// code = e4m3fn_rne(clamp(x * inv, -448, 448)): the product and the clamp in
// fp32 before the convert (overflow saturates to +-448), NaN -> sign | 0x7f.
// v_cvt_pk_fp8_f32 was checked against the integer-arithmetic definition on
// every fp32 bit pattern (DESIGN.md "fp8 KV pool"): equal on every non-NaN
// input, subnormal results included; it gives 0xff for every NaN, so the sign
// of a NaN is put back here.
__device__ __forceinline__ float e4m3_prep(float x, float inv) {
    const float y = __fmul_rn(x, inv);
    return y != y ? y : fminf(fmaxf(y, -448.0f), 448.0f);
}
__device__ __forceinline__ unsigned e4m3_nan_sign(float y, int byte) {  // bit to clear in a packed word
    return (y != y && !(__float_as_uint(y) >> 31)) ? 0x80u << (8 * byte) : 0u;
}
// four values -> four codes, value i in byte i
__device__ __forceinline__ unsigned f32x4_to_e4m3(float a, float b, float c, float d, float inv) {
    const float y0 = e4m3_prep(a, inv), y1 = e4m3_prep(b, inv), y2 = e4m3_prep(c, inv), y3 = e4m3_prep(d, inv);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(y0, y1, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y2, y3, w, true);
    return (unsigned)w & ~(e4m3_nan_sign(y0, 0) | e4m3_nan_sign(y1, 1) | e4m3_nan_sign(y2, 2) | e4m3_nan_sign(y3, 3));
}
__device__ __forceinline__ unsigned char f32_to_e4m3(float x, float inv) {
    const float y = e4m3_prep(x, inv);
    const unsigned w = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(y, y, 0, false);
    return (unsigned char)((w & ~e4m3_nan_sign(y, 0)) & 0xffu);
}
// a packed word of four codes -> their exact fp32 values (v_cvt_pk_f32_fp8)
typedef float e4m3_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 e4m3x4_to_f32(unsigned w) {
    const e4m3_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const e4m3_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// The K/V slot of the pool layout (hip_paged_attn.h), in elements of the pool's
// dtype.  A page holds [K | V][head] tiles of P slots x 64 dims: the tile of
// (kv, head) of `page` starts at kv_tile_off from the layer's base.  Within
// it K is [chunk of 16 B][slot][chunk] -- CH = 4 (fp32), 8 (bf16) or 16 (fp8)
// elements per chunk -- and V is [slot][64].  (hs: the head size, 64 in every
// kernel; the host's index functions pass the pool's.)
__host__ __device__ __forceinline__ size_t kv_tile_off(int page, const size_t& page_elems, int NH, int kv, int head,
                                                       int P, int hs = 64) {
    return (size_t)page * page_elems + ((size_t)kv * NH + head) * P * hs;
}
template <int CH>  // the chunk of dim d at `slot`
__host__ __device__ __forceinline__ int kv_k_chunk(int d, int slot, int P) {
    static_assert(CH == 4 || CH == 8 || CH == 16, "K chunks of 16 bytes: fp32, bf16 or fp8 elements");
    constexpr int SH = CH == 4 ? 2 : CH == 8 ? 3 : 4;
    return ((d >> SH) * P + slot) * CH;
}
template <int CH>
__host__ __device__ __forceinline__ int kv_k_off(int d, int slot, int P) {
    return kv_k_chunk<CH>(d, slot, P) + (d & (CH - 1));
}
__host__ __device__ __forceinline__ int kv_v_off(int d, int slot, int hs = 64) { return slot * hs + d; }
template <int CH>  // ... of K (kv = 0) or V (kv = 1)
__host__ __device__ __forceinline__ int kv_off(int kv, int d, int slot, int P) {
    return kv == 0 ? kv_k_off<CH>(d, slot, P) : kv_v_off(d, slot);
}

// The K/V stores of every decode path (add_to_cache, paged_infer.c:505-573)
// into the tile at toff = kv_tile_off(..) of the layer at `layer`: fp32 as is,
// bf16 RNE, fp8 the e4m3fn codes of val * inv (inv: the tile's entry of the
// pool's scales).  A caller computes toff once, ahead of any branch on the
// pool's dtype.
// kv_store4: dims d .. d+3 (d % 4 == 0) of one slot as one 16 B, 8 B or 4 B
// store
template <int CH>
__device__ __forceinline__ void kv_store4(void* layer, size_t toff, int kv, int d, int slot, int P, float4 v,
                                          float inv = 1.f) {
    if constexpr (CH == 4) {  // four dims are one whole fp32 chunk
        float* kvt = reinterpret_cast<float*>(layer) + toff + (kv == 0 ? kv_k_chunk<4>(d, slot, P) : kv_v_off(d, slot));
        *reinterpret_cast<float4*>(kvt) = v;
    } else if constexpr (CH == 8) {
        unsigned short* kvt = reinterpret_cast<unsigned short*>(layer) + toff + kv_off<8>(kv, d, slot, P);
        const unsigned lo = f32_to_bf16(v.x) | ((unsigned)f32_to_bf16(v.y) << 16);
        const unsigned hi = f32_to_bf16(v.z) | ((unsigned)f32_to_bf16(v.w) << 16);
        *reinterpret_cast<uint2*>(kvt) = make_uint2(lo, hi);
    } else {
        unsigned char* kvt = reinterpret_cast<unsigned char*>(layer) + toff + kv_off<16>(kv, d, slot, P);
        *reinterpret_cast<unsigned*>(kvt) = f32x4_to_e4m3(v.x, v.y, v.z, v.w, inv);
    }
}
// kv_store1: one dim; inv: fp8 pools
template <int CH>
__device__ __forceinline__ void kv_store1(void* layer, size_t toff, int kv, int d, int slot, int P, float val,
                                          float inv = 1.f) {
    if constexpr (CH == 16) {
        unsigned char* kvt = reinterpret_cast<unsigned char*>(layer) + toff;
        kvt[kv_off<16>(kv, d, slot, P)] = f32_to_e4m3(val, inv);
    } else if constexpr (CH == 8) {
        unsigned short* kvt = reinterpret_cast<unsigned short*>(layer) + toff;
        kvt[kv_off<8>(kv, d, slot, P)] = f32_to_bf16(val);
    } else {
        float* kvt = reinterpret_cast<float*>(layer) + toff;
        kvt[kv_off<4>(kv, d, slot, P)] = val;
    }
}
// kv_store1_rt: ... by the pool's run-time dtype; scales[sidx]: the tile's inv (read by fp8
// pools only).  SPLIT32: an fp32 pool's K and V as two stores under a branch
// on kv, the form the GEMM epilogues were tuned with (else one store at a
// selected address)
template <bool SPLIT32 = true>
__device__ __forceinline__ void kv_store1_rt(int dtype, void* layer, size_t toff, int kv, int d, int slot, int P, float val,
                                          const float* scales, size_t sidx) {
    if (dtype == HPA_FP8) {
        kv_store1<16>(layer, toff, kv, d, slot, P, val, scales[sidx]);
    } else if (dtype == HPA_BF16) {
        kv_store1<8>(layer, toff, kv, d, slot, P, val);
    } else if (SPLIT32) {
        if (kv == 0)
            kv_store1<4>(layer, toff, 0, d, slot, P, val);
        else
            kv_store1<4>(layer, toff, 1, d, slot, P, val);
    } else {
        kv_store1<4>(layer, toff, kv, d, slot, P, val);
    }
}

// GELU of the reference (paged_infer.c:243-251): 0.5 x (1 + tanh(sqrt(2/pi)(x + 0.044715 x^3)))
__device__ __forceinline__ float gelu_ref(float x) {
    // sqrtf(2.0f / M_PI) as the reference computes it: float(2/pi) then sqrtf
    const float s = __uint_as_float(0x3F4C4229u);  // 0.79788452
    float cube = __fmul_rn(__fmul_rn(__fmul_rn(0.044715f, x), x), x);
    return __fmul_rn(__fmul_rn(0.5f, x), __fadd_rn(1.0f, tanhf(__fmul_rn(s, __fadd_rn(x, cube)))));
}
}  // namespace hpa
