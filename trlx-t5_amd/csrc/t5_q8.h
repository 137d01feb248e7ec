// The e4m3fn quantisation the fp8 forms share: the cast, the power-of-two scale's exponent and the
// absolute maximum over bf16 bit patterns.  k_t5_cross_kv_quantize (t5_cross_kv8.hip) applies them
// to a (batch row, head) block of encoder keys, k_t5_linear_w8_quantize (t5_decode_linear_w8.hip) to
// a weight row: one rule, the same bytes for the same values and exponent.
#pragma once

#include "common.h"

namespace trlx {

// fp32 -> e4m3fn byte, round to nearest even; at or above 480 (and NaN) -> 0x7f.  torch's cast.
__device__ __forceinline__ uint32_t f32_to_e4m3fn(float f) {
    uint32_t b = __float_as_uint(f);
    const uint32_t sign = b & 0x80000000u;
    b ^= sign;
    uint32_t r;
    if (b >= (1087u << 20)) {
        r = 0x7fu;
    } else if (b < (121u << 23)) {   // below 2^-6: the subnormals, rounded by an fp32 add
        const uint32_t magic = 141u << 23;
        r = __float_as_uint(__fadd_rn(__uint_as_float(b), __uint_as_float(magic))) - magic;
    } else {
        const uint32_t odd = (b >> 20) & 1u;
        b += (uint32_t(7 - 127) << 23) + 0x7ffffu;
        b += odd;
        r = b >> 20;
    }
    return (r | (sign >> 24)) & 0xffu;
}

// the exponent e of the scale from the bf16 pattern of amax (finite): the smallest e with
// amax * 2^-e <= 448, 0 for amax == 0, clamped to [-100, 119]
__device__ __forceinline__ int q8_exponent(uint32_t amax_bits) {
    if (amax_bits == 0) return 0;
    const int E = int(amax_bits >> 7), M = int(amax_bits & 0x7fu);
    if (E == 0) return -100;                       // a bf16 subnormal: far below the clamp
    const int e = (E - 126) - (M <= 96 ? 9 : 8);   // frexp: m = (1 + M / 128) / 2 <= 0.875 iff M <= 96
    return e < -100 ? -100 : e > 119 ? 119 : e;
}

__device__ __forceinline__ uint32_t q8_absmax(const vec4u& x, uint32_t m) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m = max(m, w[i] & 0x7fffu);
        m = max(m, (w[i] >> 16) & 0x7fffu);
    }
    return m;
}

__device__ __forceinline__ uint32_t q8_pack4(uint32_t lo, uint32_t hi, float inv) {
    return f32_to_e4m3fn(__fmul_rn(bf_lo(lo), inv)) | (f32_to_e4m3fn(__fmul_rn(bf_hi(lo), inv)) << 8) |
           (f32_to_e4m3fn(__fmul_rn(bf_lo(hi), inv)) << 16) | (f32_to_e4m3fn(__fmul_rn(bf_hi(hi), inv)) << 24);
}

}  // namespace trlx
