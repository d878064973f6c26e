// hpa_mx_quant.h -- the MXFP4 weight quantisation rule (group exponent and
// e2m1 code), shared by the two fp4 packs: hpa_pack_frag_fp4 (hpa_gemm_fp4w.hip)
// and hpa_pack_frag_mx4 (hpa_gemm_mx48.hip) write the same codes and the same
// e8m0 bytes, in different layouts.
#pragma once

namespace {
// the group's exponent t from its absmax, exactly from the fp32 fields: absmax
// = (1 + f) 2^E gives t = E - 2 when 1 + f <= 1.5 (6 = 1.5 x 2^2), else E - 1,
// so absmax / 2^t lies in (3, 6].  Clamped to [-64, 64] (a zero-exponent or
// tiny absmax: -64, the group keeps what e2m1 resolves there; infinite or
// huge: 64 and the codes saturate at +-6).  An all-zero group: 0.
__device__ __forceinline__ int f4w_scale_exp(float absmax) {
    const unsigned u = __float_as_uint(absmax);
    const int ef = (int)((u >> 23) & 0xffu);
    const int t = ef == 0 ? -64 : ef - 127 - ((u & 0x7fffffu) <= 0x400000u ? 2 : 1);
    return absmax == 0.f ? 0 : max(-64, min(64, t));
}
// e2m1 code of v = w 2^-t, round to nearest, ties to the even mantissa (0.25
// -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), clamped
// at 6; bit 3 = (w < 0).  Written out in comparisons: the pack is not a hot
// path and every boundary can be read here.
__device__ __forceinline__ unsigned f4w_code(float w, float inv) {
    const float x = fabsf(w) * inv;
    const unsigned m = x <= 0.25f ? 0u : x < 0.75f ? 1u : x <= 1.25f ? 2u : x < 1.75f ? 3u
                     : x <= 2.5f ? 4u : x < 3.5f ? 5u : x <= 5.f ? 6u : 7u;
    return m | (w < 0.f ? 8u : 0u);
}
}  // namespace
