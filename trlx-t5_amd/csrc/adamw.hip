// Fused multi-tensor AdamW step with the ILQL target-head sync in the same pass (C ABI:
// trlx_adamw_step in include/trlx_t5_amd.h).
//
//   k_adamw   torch.optim.AdamW's _single_tensor_adam (decoupled decay) over a by-value table of
//             tensors in one launch: every op of the update is a separately rounded fp32 op in
//             torch's order.  p fp32 or bf16 (with or without an fp32 master), g fp32 or bf16,
//             m and v fp32.  An entry with a target also writes k_polyak's
//             target <- alpha·p_new + (1 - alpha)·target from the p just formed, so the sync never
//             re-reads the parameters.  HBM-bound: 28 B per fp32 parameter (read p, g, m, v, write
//             p, m, v), 36 B with the fold.
//
// One workgroup takes one chunk of TRLX_ADAMW_CHUNK elements of one tensor.  A tensor whose
// pointers share a 16-B phase is processed as [head | groups of G elements | tail], G = 4 (all
// fp32) or 8 (a bf16 p or g: one 16-B vector of the bf16 arrays, two of the fp32 arrays);
// otherwise element by element.  Both paths run adamw_one on the same values: alignment never
// changes a result bit.
#include <math.h>

#include "common.h"

namespace trlx {

constexpr int kAdamwThreads = 256;
constexpr int64_t kAdamwMaxGrid = 1LL << 30;

struct AdamwEntry {
    void* p;
    const void* g;
    float* m;
    float* v;
    float* master;  // NULL: none
    void* target;   // NULL: none
    int64_t n;
};
struct AdamwScalars {
    float decay, w1, b2, w2, neg_step, sqrt_bc2, eps;  // 1 - lr·wd, 1-b1, b2, 1-b2, -(lr/bc1), sqrt(bc2), eps
    float alpha, beta;                                 // alpha and 1 - alpha of the folded sync
};
struct AdamwTable {
    AdamwEntry e[TRLX_ADAMW_MAX_TENSORS];
    int blk0[TRLX_ADAMW_MAX_TENSORS + 1];  // first workgroup of each entry; [count] = the grid
    int count;
    AdamwScalars s;
};

// Host and device derive the split from the same rule.  A pointer of element size es reaches a
// 16-B boundary after h elements with h = ((16 - addr % 16) % 16) / es modulo 16 / es: the bf16
// pointers must agree modulo 8, the fp32 pointers modulo 4, and the two kinds modulo 4.
struct AdamwSplit {
    bool vec;
    int64_t head, ngrp, tail0, blocks;
    __host__ __device__ AdamwSplit(const AdamwEntry& e, int p_es, int g_es) {
        const int G = (p_es == 2 || g_es == 2) ? 8 : 4;
        const uintptr_t a[6] = {reinterpret_cast<uintptr_t>(e.p),      reinterpret_cast<uintptr_t>(e.g),
                                reinterpret_cast<uintptr_t>(e.m),      reinterpret_cast<uintptr_t>(e.v),
                                reinterpret_cast<uintptr_t>(e.master), reinterpret_cast<uintptr_t>(e.target)};
        const int es[6] = {p_es, g_es, 4, 4, 4, p_es};
        int h8 = -1, h4 = -1;
        vec = true;
        for (int i = 0; i < 6; ++i) {
            if (!a[i]) continue;
            const int h = int(((16u - unsigned(a[i] & 15u)) & 15u) / unsigned(es[i]));
            int& slot = es[i] == 2 ? h8 : h4;
            if (slot < 0) slot = h;
            else if (slot != h) vec = false;
        }
        if (h8 >= 0 && (h8 & 3) != h4) vec = false;  // m and v are always there: h4 >= 0
        blocks = (e.n + TRLX_ADAMW_CHUNK - 1) / TRLX_ADAMW_CHUNK;
        if (vec) {
            head = h8 >= 0 ? h8 : h4;
            if (head > e.n) head = e.n;
            ngrp = (e.n - head) / G;
            tail0 = head + ngrp * G;
            blocks = (ngrp + TRLX_ADAMW_CHUNK / G - 1) / (TRLX_ADAMW_CHUNK / G);
        } else {
            head = ngrp = tail0 = 0;
        }
        if (blocks < 1) blocks = 1;
    }
};

// torch's _single_tensor_adam, one element: mul_, lerp_ (weight < 0.5: a + w·(b - a)), mul_ then
// addcmul_, sqrt / div / add_, addcdiv_ — correctly rounded sqrt and divisions, no contraction.
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamwScalars& s) {
    p = mul_rn(p, s.decay);
    m = add_rn(m, mul_rn(s.w1, __fsub_rn(g, m)));
    v = add_rn(mul_rn(v, s.b2), mul_rn(s.w2, mul_rn(g, g)));
    const float denom = add_rn(__fdiv_rn(__fsqrt_rn(v), s.sqrt_bc2), s.eps);
    p = add_rn(p, mul_rn(s.neg_step, __fdiv_rn(m, denom)));
}

// k_polyak's rounding (ilql_heads.hip polyak_one): the products and, for bf16, each
// intermediate pass through the tensor's dtype; the store rounds the sum.
template <class DT>
__device__ __forceinline__ float adamw_sync_one(float src, float t, const AdamwScalars& s);
template <>
__device__ __forceinline__ float adamw_sync_one<F32T>(float src, float t, const AdamwScalars& s) {
    return add_rn(mul_rn(s.alpha, src), mul_rn(s.beta, t));
}
template <>
__device__ __forceinline__ float adamw_sync_one<BF16T>(float src, float t, const AdamwScalars& s) {
    const float a = bf2f(f2bf(mul_rn(s.alpha, src))), b = bf2f(f2bf(mul_rn(s.beta, t)));
    return add_rn(a, b);
}

// the value a store of dtype DT leaves in memory
template <class DT>
__device__ __forceinline__ float as_stored(float x);
template <>
__device__ __forceinline__ float as_stored<F32T>(float x) { return x; }
template <>
__device__ __forceinline__ float as_stored<BF16T>(float x) { return bf2f(f2bf(x)); }

// One element through scalar accesses (the head, the tail and tensors of mixed phase).
template <class PT, class GT>
__device__ __forceinline__ void adamw_elem(const AdamwEntry& e, int64_t k, const AdamwScalars& s) {
    float p = e.master ? e.master[k] : PT::load1(e.p, k);
    float m = e.m[k], v = e.v[k];
    adamw_one(p, GT::load1(e.g, k), m, v, s);
    e.m[k] = m;
    e.v[k] = v;
    if (e.master) e.master[k] = p;
    PT::store1(e.p, k, p);
    if (e.target) PT::store1(e.target, k, adamw_sync_one<PT>(as_stored<PT>(p), PT::load1(e.target, k), s));
}

// G elements of an array of dtype DT starting at 16-B aligned `base + grp·G`: one vector when
// the dtype fills 16 B with G elements, two otherwise (fp32 with G = 8).
template <class DT, int G, bool STREAM>
__device__ __forceinline__ void load_group(const void* base, int64_t grp, float (&f)[G]) {
    constexpr int NV = G / DT::kEPV;
    const vec4u* q = reinterpret_cast<const vec4u*>(base) + grp * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float t[DT::kEPV];
        DT::unpack(STREAM ? ld_stream(q + i) : q[i], t);
#pragma unroll
        for (int j = 0; j < DT::kEPV; ++j) f[i * DT::kEPV + j] = t[j];
    }
}
template <class DT, int G>
__device__ __forceinline__ void store_group(void* base, int64_t grp, const float (&f)[G]) {
    constexpr int NV = G / DT::kEPV;
    vec4u* q = reinterpret_cast<vec4u*>(base) + grp * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float t[DT::kEPV];
#pragma unroll
        for (int j = 0; j < DT::kEPV; ++j) t[j] = f[i * DT::kEPV + j];
        q[i] = DT::pack(t);
    }
}

template <class PT, class GT>
__global__ __launch_bounds__(kAdamwThreads) void k_adamw(AdamwTable t) {
    typedef typename PT::elem_t PE;
    typedef typename GT::elem_t GE;
    constexpr int G = (PT::kEPV == 8 || GT::kEPV == 8) ? 8 : 4;
    constexpr int kGroups = TRLX_ADAMW_CHUNK / G;  // groups per workgroup
    int i = 0;
    while (i + 1 < t.count && int(blockIdx.x) >= t.blk0[i + 1]) ++i;  // block-uniform
    const int64_t j = int(blockIdx.x) - t.blk0[i];
    const AdamwEntry e = t.e[i];
    const AdamwScalars s = t.s;
    const int tid = threadIdx.x;
    const AdamwSplit sp(e, int(sizeof(PE)), int(sizeof(GE)));
    if (!sp.vec) {
        const int64_t k1 = min(e.n, (j + 1) * int64_t(TRLX_ADAMW_CHUNK));
        for (int64_t k = j * int64_t(TRLX_ADAMW_CHUNK) + tid; k < k1; k += kAdamwThreads) adamw_elem<PT, GT>(e, k, s);
        return;
    }
    // every array from its first 16-B boundary (element sp.head)
    PE* pb = static_cast<PE*>(e.p) + sp.head;
    const GE* gb = static_cast<const GE*>(e.g) + sp.head;
    float *mb = e.m + sp.head, *vb = e.v + sp.head;
    float* wb = e.master ? e.master + sp.head : nullptr;
    PE* tb = e.target ? static_cast<PE*>(e.target) + sp.head : nullptr;
    const int64_t g1 = min(sp.ngrp, (j + 1) * kGroups);
#pragma unroll 2
    for (int64_t q = j * kGroups + tid; q < g1; q += kAdamwThreads) {
        float p[G], g[G], m[G], v[G];
        if (wb) load_group<F32T, G, false>(wb, q, p);
        else load_group<PT, G, false>(pb, q, p);
        load_group<GT, G, true>(gb, q, g);
        load_group<F32T, G, false>(mb, q, m);
        load_group<F32T, G, false>(vb, q, v);
#pragma unroll
        for (int k = 0; k < G; ++k) adamw_one(p[k], g[k], m[k], v[k], s);
        store_group<F32T, G>(mb, q, m);
        store_group<F32T, G>(vb, q, v);
        if (wb) store_group<F32T, G>(wb, q, p);
        store_group<PT, G>(pb, q, p);
        if (tb) {
            float tg[G];
            load_group<PT, G, false>(tb, q, tg);
#pragma unroll
            for (int k = 0; k < G; ++k) tg[k] = adamw_sync_one<PT>(as_stored<PT>(p[k]), tg[k], s);
            store_group<PT, G>(tb, q, tg);
        }
    }
    if (j == 0) {  // the < G head and tail elements
        int64_t k = -1;
        if (tid < sp.head) k = tid;
        else if (tid - sp.head < e.n - sp.tail0) k = sp.tail0 + (tid - sp.head);
        if (k >= 0) adamw_elem<PT, GT>(e, k, s);
    }
}

}  // namespace trlx

using namespace trlx;

static int adamw_launch(const AdamwTable& t, int p_dtype, int g_dtype, hipStream_t stream) {
    const dim3 grid{unsigned(t.blk0[t.count])}, block(kAdamwThreads);
    if (p_dtype == TRLX_BF16 && g_dtype == TRLX_BF16)
        hipLaunchKernelGGL((k_adamw<BF16T, BF16T>), grid, block, 0, stream, t);
    else if (p_dtype == TRLX_BF16)
        hipLaunchKernelGGL((k_adamw<BF16T, F32T>), grid, block, 0, stream, t);
    else if (g_dtype == TRLX_BF16)
        hipLaunchKernelGGL((k_adamw<F32T, BF16T>), grid, block, 0, stream, t);
    else
        hipLaunchKernelGGL((k_adamw<F32T, F32T>), grid, block, 0, stream, t);
    return check_launch("k_adamw");
}

static AdamwEntry adamw_entry(const trlx_adamw_args& a, int64_t i) {
    AdamwEntry e;
    e.p = a.p[i];
    e.g = a.g[i];
    e.m = static_cast<float*>(a.m[i]);
    e.v = static_cast<float*>(a.v[i]);
    e.master = a.master ? static_cast<float*>(a.master[i]) : nullptr;
    e.target = a.target ? a.target[i] : nullptr;
    e.n = a.numel[i];
    return e;
}

extern "C" int trlx_adamw_step(const trlx_adamw_args* args, void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_adamw_args");
    const trlx_adamw_args& a = *args;
    TRLX_REQUIRE(a.p_dtype == TRLX_F32 || a.p_dtype == TRLX_BF16, TRLX_ERR_DTYPE, "adamw parameter dtype %d", a.p_dtype);
    TRLX_REQUIRE(a.g_dtype == TRLX_F32 || a.g_dtype == TRLX_BF16, TRLX_ERR_DTYPE, "adamw gradient dtype %d", a.g_dtype);
    TRLX_REQUIRE(a.count >= 0 && (a.count == 0 || (a.p && a.g && a.m && a.v && a.numel)), TRLX_ERR_ARG,
                 "bad adamw tensor list");
    TRLX_REQUIRE(a.step >= 1, TRLX_ERR_ARG, "adamw step %lld (the first update is step 1)", (long long)a.step);
    TRLX_REQUIRE(a.lr == a.lr && a.beta1 == a.beta1 && a.beta2 == a.beta2 && a.eps == a.eps &&
                     a.weight_decay == a.weight_decay,
                 TRLX_ERR_ARG, "adamw: a NaN hyper-parameter");
    const int p_es = a.p_dtype == TRLX_BF16 ? 2 : 4, g_es = a.g_dtype == TRLX_BF16 ? 2 : 4;
    static const char* const kNames[6] = {"p", "g", "m", "v", "master", "target"};
    for (int64_t i = 0; i < a.count; ++i) {  // validate everything before the first launch
        const AdamwEntry e = adamw_entry(a, i);
        TRLX_REQUIRE(e.n >= 0, TRLX_ERR_SHAPE, "adamw tensor %lld: numel %lld", (long long)i, (long long)e.n);
        if (e.n == 0) continue;
        TRLX_REQUIRE(e.p && e.g && e.m && e.v, TRLX_ERR_ARG, "adamw tensor %lld: NULL pointer", (long long)i);
        TRLX_REQUIRE(!(e.master && a.p_dtype != TRLX_BF16), TRLX_ERR_ARG,
                     "adamw tensor %lld: a master is for a bf16 parameter", (long long)i);
        TRLX_REQUIRE(!e.target || a.alpha == a.alpha, TRLX_ERR_ARG, "adamw: alpha is NaN");
        TRLX_REQUIRE(e.n <= int64_t(TRLX_ADAMW_CHUNK) * kAdamwMaxGrid, TRLX_ERR_SHAPE,
                     "adamw tensor %lld too large (%lld elements)", (long long)i, (long long)e.n);
        const uintptr_t ptr[6] = {reinterpret_cast<uintptr_t>(e.p),      reinterpret_cast<uintptr_t>(e.g),
                                  reinterpret_cast<uintptr_t>(e.m),      reinterpret_cast<uintptr_t>(e.v),
                                  reinterpret_cast<uintptr_t>(e.master), reinterpret_cast<uintptr_t>(e.target)};
        const int es[6] = {p_es, g_es, 4, 4, 4, p_es};
        for (int x = 0; x < 6; ++x)
            TRLX_REQUIRE((ptr[x] & uintptr_t(es[x] - 1)) == 0, TRLX_ERR_ARG,
                         "adamw tensor %lld: %s not aligned to the element size", (long long)i, kNames[x]);
        for (int x = 0; x < 6; ++x)
            for (int y = x + 1; y < 6; ++y) {
                if (!ptr[x] || !ptr[y]) continue;
                const uintptr_t bx = uintptr_t(e.n) * uintptr_t(es[x]), by = uintptr_t(e.n) * uintptr_t(es[y]);
                TRLX_REQUIRE(ptr[x] + bx <= ptr[y] || ptr[y] + by <= ptr[x], TRLX_ERR_ARG,
                             "adamw tensor %lld: %s and %s alias", (long long)i, kNames[x], kNames[y]);
            }
    }
    // the scalars, formed in double as torch forms them, rounded to fp32 once
    const double bc1 = 1.0 - pow(a.beta1, double(a.step)), bc2 = 1.0 - pow(a.beta2, double(a.step));
    AdamwTable t;
    t.s.decay = float(1.0 - a.lr * a.weight_decay);
    t.s.w1 = float(1.0 - a.beta1);
    t.s.b2 = float(a.beta2);
    t.s.w2 = float(1.0 - a.beta2);
    t.s.neg_step = float(-(a.lr / bc1));
    t.s.sqrt_bc2 = float(sqrt(bc2));
    t.s.eps = float(a.eps);
    t.s.alpha = float(a.alpha);
    t.s.beta = float(1.0 - a.alpha);
    t.count = 0;
    t.blk0[0] = 0;
    for (int64_t i = 0; i < a.count; ++i) {
        const AdamwEntry e = adamw_entry(a, i);
        if (e.n == 0) continue;  // zero-length tensors are skipped
        const int64_t blocks = AdamwSplit(e, p_es, g_es).blocks;
        if (t.count == TRLX_ADAMW_MAX_TENSORS || t.blk0[t.count] + blocks > kAdamwMaxGrid) {
            const int rc = adamw_launch(t, a.p_dtype, a.g_dtype, (hipStream_t)stream);
            if (rc) return rc;
            t.count = 0;
        }
        t.e[t.count] = e;
        t.blk0[t.count + 1] = int(t.blk0[t.count] + blocks);
        ++t.count;
    }
    return t.count ? adamw_launch(t, a.p_dtype, a.g_dtype, (hipStream_t)stream) : TRLX_OK;
}
