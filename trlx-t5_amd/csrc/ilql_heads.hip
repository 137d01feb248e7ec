// ILQL heads: the target-Q heads evaluated at the action tokens only, and the Polyak sync of
// the target heads (C ABI: trlx_ilql_tq_at_actions, trlx_polyak_update in
// include/trlx_t5_amd.h).
//
//   k_ilql_tq_at_actions  ILQLConfig.loss reads one scalar per (b, a) from each target-Q
//                    tensor — tq_i[b, a, a*], a* = input_ids[b, 1 + actions_ixs[b, a]]
//                    (ilql_rows.hip) — so the second layer of a target head
//                    (ilql_models.py:31-34,156) is only needed at a*: a gathered row dot
//                    z[b, a, :] · W2[a*, :] + b2[a*].  One wave per (token, head): 16-B loads
//                    of both rows, fp32 accumulators, a shuffle reduction; no LDS, no atomics.
//                    HBM: 2·K·s bytes per (token, head) instead of the [B, A, V] GEMM.
//   k_polyak         target <- alpha·src + (1 - alpha)·target (ilql_models.py:161-168) over a
//                    table of tensors in one launch, rounded as torch's three elementwise ops.
#include <algorithm>

#include "common.h"

namespace trlx {

constexpr int kTqWaves = 4;  // waves (= (token, head) pairs) per workgroup

// The summation order is a function of (K, dtype) alone: element k belongs to 16-B vector
// v = k / EPV, which lane v % 64 takes at step v / 64; a lane keeps one fp32 accumulator per
// element slot e = k % EPV (fma chains over the steps), adds its slots in a fixed tree, and
// the wave adds the lanes in a fixed butterfly.  The vector and the scalar path load the same
// elements into the same chains, so alignment never changes a result bit.
template <class DT, bool VEC>
__device__ __forceinline__ float tq_row_dot(const typename DT::elem_t* z, const typename DT::elem_t* w, int64_t K,
                                            int lane) {
    constexpr int EPV = DT::kEPV;
    float acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.0f;
    const int64_t nvec = (K + EPV - 1) / EPV;
    if constexpr (VEC) {  // K % EPV == 0, both rows 16-B aligned
        const vec4u* zv = reinterpret_cast<const vec4u*>(z);
        const vec4u* wv = reinterpret_cast<const vec4u*>(w);
#pragma unroll 4
        for (int64_t v = lane; v < nvec; v += kWave) {
            float fz[EPV], fw[EPV];
            DT::unpack(zv[v], fz);
            DT::unpack(wv[v], fw);
#pragma unroll
            for (int e = 0; e < EPV; ++e) acc[e] = fmaf(fz[e], fw[e], acc[e]);
        }
    } else {
        for (int64_t v = lane; v < nvec; v += kWave) {
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                const int64_t k = v * EPV + e;
                if (k < K) acc[e] = fmaf(DT::load1(z, k), DT::load1(w, k), acc[e]);
            }
        }
    }
#pragma unroll
    for (int width = EPV / 2; width > 0; width /= 2)
#pragma unroll
        for (int e = 0; e < width; ++e) acc[e] = add_rn(acc[e], acc[e + width]);
    return wave_sum(acc[0]);
}

template <class DT>
__global__ __launch_bounds__(kTqWaves* kWave) void k_ilql_tq_at_actions(trlx_ilql_tq_args a) {
    typedef typename DT::elem_t E;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t N = a.B * a.A;
    const int64_t job = int64_t(blockIdx.x) * kTqWaves + threadIdx.x / kWave;  // wave-uniform
    if (job >= N * a.nh) return;
    const int h = int(job / N);
    const int64_t n = job - int64_t(h) * N;
    const int64_t b = n / a.A, t = n - b * a.A;
    // a* exactly as k_ilql_rows computes it (no out-of-bounds gather)
    const int64_t ix = a.actions_ixs[b * a.A + t];
    const int64_t y = (ix >= 0 && ix < a.L - 1) ? a.input_ids[b * a.L + 1 + ix] : -1;
    float* out = a.out[h] + n;
    if (!(y >= 0 && y < a.V)) {  // as y_ok in the loss: NaN, nothing read
        if (lane == 0) *out = NAN;
        return;
    }
    const E* z = static_cast<const E*>(a.z[h]) + b * a.z_sb[h] + t * a.z_st[h];
    const E* w = static_cast<const E*>(a.w2[h]) + y * a.w2_ld[h];
    const bool vec = a.K % DT::kEPV == 0 &&
                     ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(w)) & 15u) == 0;
    const float s = vec ? tq_row_dot<DT, true>(z, w, a.K, lane) : tq_row_dot<DT, false>(z, w, a.K, lane);
    if (lane == 0) *out = a.b2[h] ? add_rn(s, DT::load1(a.b2[h], y)) : s;
}

// ------------------------------------------------------------------ Polyak update
constexpr int kPolyakThreads = 256;
constexpr int kPolyakVecs = 2048;  // 16-B vectors per workgroup (8 per thread)

struct PolyakEntry {
    const void* src;
    void* dst;
    int64_t n;
};
struct PolyakTable {
    PolyakEntry e[TRLX_POLYAK_MAX_TENSORS];
    int blk0[TRLX_POLYAK_MAX_TENSORS + 1];  // first workgroup of each entry; [count] = the grid
    int count;
    float alpha, beta;  // alpha and 1 - alpha (formed in double), each rounded to fp32
};

// A tensor whose source and target share a 16-B phase is processed as [head | 16-B body |
// tail]; otherwise element by element.  Host and device derive the split from the same rule.
struct PolyakSplit {
    bool vec;
    int64_t head, nvec, tail0, blocks;
    __host__ __device__ PolyakSplit(const void* src, const void* dst, int64_t n, int es) {
        const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
        const int epv = 16 / es;
        vec = ((s ^ d) & 15u) == 0;
        if (vec) {
            head = int64_t(((16u - (s & 15u)) & 15u) / unsigned(es));
            if (head > n) head = n;
            nvec = (n - head) / epv;
            tail0 = head + nvec * epv;
            blocks = (nvec + kPolyakVecs - 1) / kPolyakVecs;
            if (blocks < 1) blocks = 1;
        } else {
            head = 0;
            nvec = 0;
            tail0 = 0;
            blocks = (n + int64_t(kPolyakVecs) * epv - 1) / (int64_t(kPolyakVecs) * epv);
        }
    }
};

// torch's `(alpha * s) + (1.0 - alpha) * t`: two separately rounded products and their sum,
// each rounded to the tensor's dtype (bf16: the products and the sum pass through bf16).
template <class DT>
__device__ __forceinline__ float polyak_one(float s, float t, float alpha, float beta);
template <>
__device__ __forceinline__ float polyak_one<F32T>(float s, float t, float alpha, float beta) {
    return add_rn(mul_rn(alpha, s), mul_rn(beta, t));
}
template <>
__device__ __forceinline__ float polyak_one<BF16T>(float s, float t, float alpha, float beta) {
    const float p = bf2f(f2bf(mul_rn(alpha, s))), q = bf2f(f2bf(mul_rn(beta, t)));
    return add_rn(p, q);  // rounded to bf16 by the store
}

template <class DT>
__global__ __launch_bounds__(kPolyakThreads) void k_polyak(PolyakTable p) {
    typedef typename DT::elem_t E;
    constexpr int EPV = DT::kEPV;
    int i = 0;
    while (i + 1 < p.count && int(blockIdx.x) >= p.blk0[i + 1]) ++i;  // block-uniform
    const int64_t j = int(blockIdx.x) - p.blk0[i];
    const E* src = static_cast<const E*>(p.e[i].src);
    E* dst = static_cast<E*>(p.e[i].dst);
    const int64_t n = p.e[i].n;
    const int tid = threadIdx.x;
    const PolyakSplit sp(src, dst, n, int(sizeof(E)));
    if (!sp.vec) {
        const int64_t per = int64_t(kPolyakVecs) * EPV;
        const int64_t k1 = min(n, (j + 1) * per);
        for (int64_t k = j * per + tid; k < k1; k += kPolyakThreads)
            DT::store1(dst, k, polyak_one<DT>(DT::load1(src, k), DT::load1(dst, k), p.alpha, p.beta));
        return;
    }
    const vec4u* sv = reinterpret_cast<const vec4u*>(src + sp.head);
    vec4u* dv = reinterpret_cast<vec4u*>(dst + sp.head);
    const int64_t v1 = min(sp.nvec, (j + 1) * kPolyakVecs);
#pragma unroll 4
    for (int64_t v = j * kPolyakVecs + tid; v < v1; v += kPolyakThreads) {
        float fs[EPV], ft[EPV];
        DT::unpack(ld_stream(sv + v), fs);
        DT::unpack(dv[v], ft);
#pragma unroll
        for (int e = 0; e < EPV; ++e) ft[e] = polyak_one<DT>(fs[e], ft[e], p.alpha, p.beta);
        dv[v] = DT::pack(ft);
    }
    if (j == 0) {  // the < EPV head and tail elements
        int64_t k = -1;
        if (tid < sp.head) k = tid;
        else if (tid - sp.head < n - sp.tail0) k = sp.tail0 + (tid - sp.head);
        if (k >= 0) DT::store1(dst, k, polyak_one<DT>(DT::load1(src, k), DT::load1(dst, k), p.alpha, p.beta));
    }
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_ilql_tq_at_actions(const trlx_ilql_tq_args* args, void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_ilql_tq_args");
    const trlx_ilql_tq_args& a = *args;
    TRLX_REQUIRE(a.dtype == TRLX_F32 || a.dtype == TRLX_BF16, TRLX_ERR_DTYPE, "target-Q heads dtype %d", a.dtype);
    TRLX_REQUIRE(a.nh == 1 || a.nh == 2, TRLX_ERR_ARG, "nh must be 1 or 2 (got %d)", a.nh);
    TRLX_REQUIRE(a.B > 0 && a.L >= 1 && a.A >= 1 && a.K >= 1 && a.V > 0, TRLX_ERR_SHAPE,
                 "bad target-Q shape B=%lld L=%lld A=%lld K=%lld V=%lld", (long long)a.B, (long long)a.L,
                 (long long)a.A, (long long)a.K, (long long)a.V);
    TRLX_REQUIRE(a.input_ids && a.actions_ixs, TRLX_ERR_ARG, "NULL input_ids / actions_ixs");
    const uintptr_t emask = a.dtype == TRLX_BF16 ? 1u : 3u;
    for (int h = 0; h < a.nh; ++h) {
        TRLX_REQUIRE(a.z[h] && a.w2[h] && a.out[h], TRLX_ERR_ARG, "NULL z / W2 / out pointer (head %d)", h);
        TRLX_REQUIRE(((reinterpret_cast<uintptr_t>(a.z[h]) | reinterpret_cast<uintptr_t>(a.w2[h]) |
                       reinterpret_cast<uintptr_t>(a.b2[h])) & emask) == 0,
                     TRLX_ERR_ARG, "z / W2 / b2 not aligned to their element size (head %d)", h);
        TRLX_REQUIRE(a.w2_ld[h] >= a.K && a.z_st[h] >= 0 && a.z_sb[h] >= 0, TRLX_ERR_STRIDE,
                     "bad z / W2 strides (head %d)", h);
    }
    const int64_t jobs = a.B * a.A * a.nh;
    const int64_t nblk = (jobs + kTqWaves - 1) / kTqWaves;
    TRLX_REQUIRE(nblk <= 0x7fffffffLL, TRLX_ERR_SHAPE, "too many tokens");
    const dim3 grid{unsigned(nblk)}, block(kTqWaves * kWave);
    if (a.dtype == TRLX_BF16)
        hipLaunchKernelGGL(k_ilql_tq_at_actions<BF16T>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_ilql_tq_at_actions<F32T>, grid, block, 0, (hipStream_t)stream, a);
    return check_launch("k_ilql_tq_at_actions");
}

static int polyak_launch(const PolyakTable& t, int dtype, hipStream_t stream) {
    const dim3 grid{unsigned(t.blk0[t.count])}, block(kPolyakThreads);
    if (dtype == TRLX_BF16)
        hipLaunchKernelGGL(k_polyak<BF16T>, grid, block, 0, stream, t);
    else
        hipLaunchKernelGGL(k_polyak<F32T>, grid, block, 0, stream, t);
    return check_launch("k_polyak");
}

extern "C" int trlx_polyak_update(const void* const* src, void* const* target, const int64_t* numel, int64_t count,
                                  int dtype, double alpha, void* stream) {
    TRLX_REQUIRE(dtype == TRLX_F32 || dtype == TRLX_BF16, TRLX_ERR_DTYPE, "polyak dtype %d", dtype);
    TRLX_REQUIRE(count >= 0 && (count == 0 || (src && target && numel)), TRLX_ERR_ARG, "bad polyak tensor list");
    TRLX_REQUIRE(alpha == alpha, TRLX_ERR_ARG, "alpha is NaN");
    const int es = dtype == TRLX_BF16 ? 2 : 4;
    constexpr int64_t kMaxGrid = 1LL << 30;
    for (int64_t i = 0; i < count; ++i) {  // validate everything before the first launch
        TRLX_REQUIRE(numel[i] >= 0, TRLX_ERR_SHAPE, "polyak tensor %lld: numel %lld", (long long)i, (long long)numel[i]);
        if (numel[i] == 0) continue;
        const uintptr_t s = reinterpret_cast<uintptr_t>(src[i]), d = reinterpret_cast<uintptr_t>(target[i]);
        TRLX_REQUIRE(s && d, TRLX_ERR_ARG, "polyak tensor %lld: NULL pointer", (long long)i);
        TRLX_REQUIRE(((s | d) & uintptr_t(es - 1)) == 0, TRLX_ERR_ARG,
                     "polyak tensor %lld: pointer not aligned to the element size", (long long)i);
        const uintptr_t bytes = uintptr_t(numel[i]) * uintptr_t(es);
        TRLX_REQUIRE(s + bytes <= d || d + bytes <= s, TRLX_ERR_ARG,
                     "polyak tensor %lld: source and target alias", (long long)i);
        TRLX_REQUIRE(PolyakSplit(src[i], target[i], numel[i], es).blocks <= kMaxGrid, TRLX_ERR_SHAPE,
                     "polyak tensor %lld too large", (long long)i);
    }
    PolyakTable t;
    t.count = 0;
    t.blk0[0] = 0;
    t.alpha = float(alpha);
    t.beta = float(1.0 - alpha);
    for (int64_t i = 0; i < count; ++i) {
        if (numel[i] == 0) continue;  // zero-length tensors are skipped
        const int64_t blocks = PolyakSplit(src[i], target[i], numel[i], es).blocks;
        if (t.count == TRLX_POLYAK_MAX_TENSORS || t.blk0[t.count] + blocks > kMaxGrid) {
            const int rc = polyak_launch(t, dtype, (hipStream_t)stream);
            if (rc) return rc;
            t.count = 0;
        }
        t.e[t.count].src = src[i];
        t.e[t.count].dst = target[i];
        t.e[t.count].n = numel[i];
        t.blk0[t.count + 1] = int(t.blk0[t.count] + blocks);
        ++t.count;
    }
    return t.count ? polyak_launch(t, dtype, (hipStream_t)stream) : TRLX_OK;
}
