// hpa_split3.h -- an fp32 value as three bf16 pieces, for kernels that keep
// fp32-class arithmetic on the bf16 matrix pipe (hpa_prefill_packed.hip,
// hpa_prefill_split.hip, hpa_gemm_split.hip).  Piece 0 = hi = the top 16 bits of
// x, 1 = mid = the top 16 bits of x - hi, 2 = lo = x - hi - mid.  Each
// difference is exact (Sterbenz: the operands agree in their leading bits), lo
// has at most 8 significant bits left, so x = hi + mid + lo exactly;
// |mid| < 2^-7 |x| and |lo| < 2^-15 |x| (truncation).
#pragma once
#include <hip/hip_runtime.h>

namespace hpa_split {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// x = pc[0] + pc[1] + pc[2] exactly, each a bf16 (the top 16 bits of the words)
__device__ __forceinline__ void split3(float x, unsigned* pc) {
    pc[0] = __float_as_uint(x) & 0xffff0000u;
    const float r = x - __uint_as_float(pc[0]);
    pc[1] = __float_as_uint(r) & 0xffff0000u;
    pc[2] = __float_as_uint(r - __uint_as_float(pc[1]));
}
__device__ __forceinline__ unsigned pack_hi16(unsigned even, unsigned odd) { return (even >> 16) | (odd & 0xffff0000u); }

// 8 fp32 values -> the bf16x8 operands of their three pieces (as dwords of pairs)
__device__ __forceinline__ void split3x8(const float* x, u32x4* piece) {
    unsigned pc[8][3];
#pragma unroll
    for (int i = 0; i < 8; ++i) split3(x[i], pc[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        piece[j] = u32x4{pack_hi16(pc[0][j], pc[1][j]), pack_hi16(pc[2][j], pc[3][j]), pack_hi16(pc[4][j], pc[5][j]),
                         pack_hi16(pc[6][j], pc[7][j])};
}

}  // namespace hpa_split
