// The per-element arithmetic the T5 row kernels share: the feed-forward activation of t5_ff_act.hip
// and the sum of squares / reciprocal root of t5_rmsnorm.hip.  t5_decode_linear.hip runs the same
// functions in its prologue and epilogue, so its results carry the bits of those kernels.
#pragma once

#include "common.h"

namespace trlx {

constexpr float kGeluC = 0.044715f;
constexpr float kGelu3C = 3.f * 0.044715f;
constexpr float kGelu2K = 1.5957691216057308f;                 // 2 sqrt(2 / pi)

// a = act(u) and, with GRAD, d = act'(u)
template <int ACT, bool GRAD>
__device__ __forceinline__ void fa_eval(float u, float& a, float& d) {
    if constexpr (ACT == TRLX_T5_ACT_RELU) {
        a = u <= 0.f ? 0.f : u;                                // NaN stays NaN
        if (GRAD) d = u > 0.f ? 1.f : (u <= 0.f ? 0.f : u);
    } else {
        float x, xp;                                           // sigmoid's argument and dx/du
        if constexpr (ACT == TRLX_T5_ACT_SILU) {
            x = u;
            xp = 1.f;
        } else {
            const float u2 = u * u;
            x = kGelu2K * (u * (1.f + kGeluC * u2));
            xp = kGelu2K * (1.f + kGelu3C * u2);
        }
        const float e = exp2_fast(-fabsf(x) * kLog2e);
        const float r = __builtin_amdgcn_rcpf(1.f + e);
        const float s = x >= 0.f ? r : e * r;
        a = u * s;
        if (GRAD) {
            const float t = e * (r * r);                       // sigmoid'(x); 0 once |x| > ~88
            const float w = t > 0.f ? (u * xp) * t : 0.f;      // u x' may be inf where t is 0
            d = s + w;                                         // NaN u: s is NaN
        }
    }
}

template <int E>
__device__ __forceinline__ float rn_sumsq(const float (&f)[E]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) s += f[i] * f[i];
    return s;
}

__device__ __forceinline__ float rn_rstd(float sumsq, int D, float eps) { return 1.f / sqrtf(sumsq / float(D) + eps); }

}  // namespace trlx
