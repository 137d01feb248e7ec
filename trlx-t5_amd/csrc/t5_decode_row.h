// The arithmetic the row-per-lane-group decode attention kernels share: k_t5_decode_attn
// (t5_decode_attn.hip), k_t5_decode_attn_group (t5_decode_attn_group.hip) and
// k_t5_decode_attn_split_part (t5_decode_attn_split.hip).  The units and their code objects stay
// separate; the geometry, the per-key step, the merge of the lane groups and the stores are written
// here once, so the bits one kernel produces for a query are the bits of the others: grouped ==
// plain on the expanded tensors, split with one live range == grouped.  k_t5_decode_attn_kv8
// (t5_cross_kv8.hip) takes the geometry and the stores and keeps a step and a merge of its own, and so
// does k_t5_decode_attn_kv8_d256 (t5_cross_kv8_d256.hip), whose step takes four keys at a time.
#pragma once

#include "common.h"

namespace trlx {

constexpr int kT5RowThreads = 256;
constexpr int kT5RowWaves = kT5RowThreads / kWave;

// A key row is DKV elements, each lane takes one 16-byte vector of EPV of them.
template <int EPV, int DKV>
struct T5RowGeom {
    static constexpr int LPR = DKV / EPV;             // lanes per key row: a lane group
    static constexpr int KPW = kWave / LPR;           // key rows per wave-wide load
    static constexpr int NG = kT5RowWaves * KPW;      // groups per workgroup
    static_assert(DKV % EPV == 0 && kWave % LPR == 0 && LPR >= 2, "row geometry");
    static_assert(DKV / 2 <= kT5RowThreads, "the merge and the zero store take d_kv / 2 threads");
};

// What a kernel adds to a score between the dot product and the softmax.  T5ScoreAdd{0.f} is not a
// no-op: it turns -0.f into +0.f, as the bias add of the self-attention does.
struct T5ScoreAdd {
    float b;
    __device__ __forceinline__ float operator()(float s) const { return s + b; }
};

// One key applied to one query: fp32 dot over the row (butterfly inside the lane group), the score
// adjustment, the online max / sum, P·V.  kf / vf are the key / value row slices unpacked to fp32.
template <int LPR, int EPV, class Adjust>
__device__ __forceinline__ void t5_row_step(const float (&qf)[EPV], const float (&kf)[EPV], const float (&vf)[EPV],
                                            float& m, float& l, float (&acc)[EPV], Adjust adjust) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EPV; ++e) s = fmaf(qf[e], kf[e], s);
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
    s = adjust(s);
    const float mn = fmaxf(m, s);
    const float sc = expf(m - mn), p = expf(s - mn);
    l = fmaf(l, sc, p);
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = fmaf(acc[e], sc, p * vf[e]);
    m = mn;
}

// Every group parks (m, l, its slice of P·V) of one query in LDS ...
template <int DKV, int EPV>
__device__ __forceinline__ void t5_row_park(float* s_m, float* s_l, float* s_acc, int gg, int sl, float m, float l,
                                            const float (&acc)[EPV]) {
#pragma unroll
    for (int e = 0; e < EPV; ++e) s_acc[gg * DKV + sl * EPV + e] = acc[e];
    if (sl == 0) {
        s_m[gg] = m;
        s_l[gg] = l;
    }
}

// ... and, after a barrier, the thread of outputs d, d + 1 combines the groups in group order.  The
// state comes back undivided; the finish is the caller's.
struct T5RowState {
    float M, L, o0, o1;
};
template <int NG, int DKV>
__device__ __forceinline__ T5RowState t5_row_merge(const float* s_m, const float* s_l, const float* s_acc, int d) {
    T5RowState r = {s_m[0], 0.f, 0.f, 0.f};
    for (int g = 1; g < NG; ++g) r.M = fmaxf(r.M, s_m[g]);
    for (int g = 0; g < NG; ++g) {
        const float mg = s_m[g];
        if (mg == -INFINITY) continue;   // a group that saw no live key
        const float w = expf(mg - r.M);
        r.L = fmaf(s_l[g], w, r.L);
        r.o0 = fmaf(s_acc[g * DKV + d], w, r.o0);
        r.o1 = fmaf(s_acc[g * DKV + d + 1], w, r.o1);
    }
    return r;
}

// o / L; no live key at all (a fully masked row): zeros.  A NaN L stays NaN.
__device__ __forceinline__ void t5_row_divide(float L, float& o0, float& o1) {
    const bool any = L > 0.f || L != L;
    o0 = any ? o0 / L : 0.f;
    o1 = any ? o1 / L : 0.f;
}

// two outputs at element offset o: a bf16 pair, rounded here, or a float2
template <class E>
__device__ __forceinline__ void t5_store_pair(void* out, int64_t o, float o0, float o1) {
    if (sizeof(E) == 2) {
        *reinterpret_cast<uint32_t*>(static_cast<uint16_t*>(out) + o) = pack_bf2(o0, o1);
    } else {
        float2 r;
        r.x = o0;
        r.y = o1;
        *reinterpret_cast<float2*>(static_cast<float*>(out) + o) = r;
    }
}

// zeros to the DKV outputs at element offset o: what a dead step and a skipped row store
template <class E, int DKV>
__device__ __forceinline__ void t5_zero_row(void* out, int64_t o) {
    if (threadIdx.x < DKV / 2) t5_store_pair<E>(out, o + 2 * threadIdx.x, 0.f, 0.f);
}

}  // namespace trlx
