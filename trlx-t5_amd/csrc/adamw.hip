// Fused multi-tensor AdamW step with the ILQL target-head sync in the same pass (C ABI:
// trlx_adamw_step in include/trlx_t5_amd.h).
//
//   k_adamw   torch.optim.AdamW's _single_tensor_adam (decoupled decay) over a by-value table of
//             tensors in one launch: every op of the update is a separately rounded fp32 op in
//             torch's order.  p fp32 or bf16 (with or without an fp32 master), g fp32 or bf16,
//             m and v fp32 (ST = F32T).  ST = BF16T (trlx_adamw_step_ex, bf16 p and g, no master):
//             m and v are bf16 and every op of the update is rounded to bf16, as torch's own
//             AdamW leaves a bf16 parameter — 14 B per parameter, every array one 16-B vector
//             per group of 8.  An entry with a target also writes k_polyak's
//             target <- alpha·p_new + (1 - alpha)·target from the p just formed, so the sync never
//             re-reads the parameters.  HBM-bound: 28 B per fp32 parameter (read p, g, m, v, write
//             p, m, v), 36 B with the fold.  The clipped instantiation (trlx_adamw_step_clipped)
//             feeds g·coef, coef read from a device record, and leaves g as it is.
//   k_grad_sumsq, k_grad_norm_finish, k_grad_scale
//             torch's clip_grad_norm_ (C ABI: trlx_grad_norm): Σ g² over a by-value table of fp32 /
//             bf16 gradients in fp64, one partial per workgroup; one small launch that adds the
//             partials in a fixed order and writes {norm, coef, nonfinite, sumsq}; the in-place
//             g <- g·coef of the stand-alone clip.  The fold costs one more read of g (+4 B per
//             fp32 parameter) where the two-call route costs +12 B.
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
    void* m;        // fp32, or bf16 with a bf16 state
    void* v;
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
// s_es: the element size of m and v.
struct AdamwSplit {
    bool vec;
    int64_t head, ngrp, tail0, blocks;
    __host__ __device__ AdamwSplit(const AdamwEntry& e, int p_es, int g_es, int s_es) {
        const int G = (p_es == 2 || g_es == 2) ? 8 : 4;
        const uintptr_t a[6] = {reinterpret_cast<uintptr_t>(e.p),      reinterpret_cast<uintptr_t>(e.g),
                                reinterpret_cast<uintptr_t>(e.m),      reinterpret_cast<uintptr_t>(e.v),
                                reinterpret_cast<uintptr_t>(e.master), reinterpret_cast<uintptr_t>(e.target)};
        const int es[6] = {p_es, g_es, s_es, s_es, 4, p_es};
        int h8 = -1, h4 = -1;
        vec = true;
        for (int i = 0; i < 6; ++i) {
            if (!a[i]) continue;
            const int h = int(((16u - unsigned(a[i] & 15u)) & 15u) / unsigned(es[i]));
            int& slot = es[i] == 2 ? h8 : h4;
            if (slot < 0) slot = h;
            else if (slot != h) vec = false;
        }
        // an fp32 state: m and v are always there, h4 >= 0; a bf16 state without a master has no
        // 4-byte array at all (h4 < 0)
        if (h8 >= 0 && (s_es == 4 || h4 >= 0) && (h8 & 3) != h4) vec = false;
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
template <class ST>
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamwScalars& s);
template <>
__device__ __forceinline__ void adamw_one<F32T>(float& p, float g, float& m, float& v, const AdamwScalars& s) {
    p = mul_rn(p, s.decay);
    m = add_rn(m, mul_rn(s.w1, __fsub_rn(g, m)));
    v = add_rn(mul_rn(v, s.b2), mul_rn(s.w2, mul_rn(g, g)));
    const float denom = add_rn(__fdiv_rn(__fsqrt_rn(v), s.sqrt_bc2), s.eps);
    p = add_rn(p, mul_rn(s.neg_step, __fdiv_rn(m, denom)));
}

// The same ops on bf16 tensors (p, g, m, v all bf16-representable on entry): torch computes each
// op in fp32 and rounds its result to bf16, so every line below ends in one rounding; inside
// lerp_, addcmul_ and addcdiv_ the products and the quotient stay fp32.
__device__ __forceinline__ float bf_rn(float x) { return bf2f(f2bf(x)); }
template <>
__device__ __forceinline__ void adamw_one<BF16T>(float& p, float g, float& m, float& v, const AdamwScalars& s) {
    p = bf_rn(mul_rn(p, s.decay));
    m = bf_rn(add_rn(m, mul_rn(s.w1, __fsub_rn(g, m))));
    v = bf_rn(mul_rn(v, s.b2));
    v = bf_rn(add_rn(v, mul_rn(s.w2, mul_rn(g, g))));
    float d = bf_rn(__fsqrt_rn(v));
    d = bf_rn(__fdiv_rn(d, s.sqrt_bc2));
    d = bf_rn(add_rn(d, s.eps));
    p = bf_rn(add_rn(p, mul_rn(s.neg_step, __fdiv_rn(m, d))));
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
// CLIP: the gradient is g·coef as a store of dtype GT would leave it (k_grad_scale's value);
// coef arrives already rounded to GT.
template <class PT, class GT, class ST, bool CLIP>
__device__ __forceinline__ void adamw_elem(const AdamwEntry& e, int64_t k, const AdamwScalars& s, float coef) {
    float p = e.master ? e.master[k] : PT::load1(e.p, k);
    float m = ST::load1(e.m, k), v = ST::load1(e.v, k);
    float g = GT::load1(e.g, k);
    if (CLIP) g = as_stored<GT>(mul_rn(g, coef));
    adamw_one<ST>(p, g, m, v, s);
    ST::store1(e.m, k, m);
    ST::store1(e.v, k, v);
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

// DEV: the scalars come from the device schedule record (trlx_adamw_advance wrote it) instead
// of the by-value table: uniform loads from a kernel-argument pointer, so they sit in SGPRs as
// t.s does.  apply == 0: the workgroup leaves before its first load of a tensor; sync == 0: the
// entry is taken without its target (the split stays the host's, which counted the target).
// ST: the dtype of m and v; BF16T comes with PT = GT = BF16T and no master only.
template <class PT, class GT, class ST = F32T, bool CLIP = false, bool DEV = false>
__global__ __launch_bounds__(kAdamwThreads) void k_adamw(AdamwTable t, const trlx_grad_norm_record* rec,
                                                         const trlx_adamw_sched* __restrict__ sched) {
    typedef typename PT::elem_t PE;
    typedef typename GT::elem_t GE;
    typedef typename ST::elem_t SE;
    constexpr int G = (PT::kEPV == 8 || GT::kEPV == 8) ? 8 : 4;
    constexpr int kGroups = TRLX_ADAMW_CHUNK / G;  // groups per workgroup
    if (DEV && sched->apply == 0) return;  // a skipped update: block-uniform
    int i = 0;
    while (i + 1 < t.count && int(blockIdx.x) >= t.blk0[i + 1]) ++i;  // block-uniform
    const int64_t j = int(blockIdx.x) - t.blk0[i];
    AdamwEntry e = t.e[i];
    const AdamwSplit sp(e, int(sizeof(PE)), int(sizeof(GE)), int(sizeof(SE)));
    if (DEV && sched->sync == 0) e.target = nullptr;
    const AdamwScalars s = DEV ? AdamwScalars{sched->decay, sched->w1, sched->b2, sched->w2, sched->neg_step,
                                              sched->sqrt_bc2, sched->eps, sched->alpha, sched->beta}
                               : t.s;
    // torch multiplies a tensor by a 0-d device tensor in the tensor's dtype: a bf16 gradient
    // meets the coefficient rounded to bf16 (fp32 product, rounded to bf16 once more)
    const float coef = CLIP ? as_stored<GT>(rec->coef) : 1.f;
    const int tid = threadIdx.x;
    if (!sp.vec) {
        const int64_t k1 = min(e.n, (j + 1) * int64_t(TRLX_ADAMW_CHUNK));
        for (int64_t k = j * int64_t(TRLX_ADAMW_CHUNK) + tid; k < k1; k += kAdamwThreads)
            adamw_elem<PT, GT, ST, CLIP>(e, k, s, coef);
        return;
    }
    // every array from its first 16-B boundary (element sp.head)
    PE* pb = static_cast<PE*>(e.p) + sp.head;
    const GE* gb = static_cast<const GE*>(e.g) + sp.head;
    SE *mb = static_cast<SE*>(e.m) + sp.head, *vb = static_cast<SE*>(e.v) + sp.head;
    float* wb = e.master ? e.master + sp.head : nullptr;
    PE* tb = e.target ? static_cast<PE*>(e.target) + sp.head : nullptr;
    const int64_t g1 = min(sp.ngrp, (j + 1) * kGroups);
#pragma unroll 2
    for (int64_t q = j * kGroups + tid; q < g1; q += kAdamwThreads) {
        float p[G], g[G], m[G], v[G];
        if (wb) load_group<F32T, G, false>(wb, q, p);
        else load_group<PT, G, false>(pb, q, p);
        load_group<GT, G, true>(gb, q, g);
        load_group<ST, G, false>(mb, q, m);
        load_group<ST, G, false>(vb, q, v);
        if (CLIP) {
#pragma unroll
            for (int k = 0; k < G; ++k) g[k] = as_stored<GT>(mul_rn(g[k], coef));
        }
#pragma unroll
        for (int k = 0; k < G; ++k) adamw_one<ST>(p[k], g[k], m[k], v[k], s);
        store_group<ST, G>(mb, q, m);
        store_group<ST, G>(vb, q, v);
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
        if (k >= 0) adamw_elem<PT, GT, ST, CLIP>(e, k, s, coef);
    }
}

// ------------------------------------------------------------------ device-resident schedule
// b^n by square-and-multiply over the bits of n from the lowest, every product a separately
// rounded fp64 multiplication (this file is built with -ffp-contract=off): a chain a CPU can
// restate bit for bit, which it cannot do for another library's pow.
__host__ __device__ inline double pow_chain(double b, int64_t n) {
    double r = 1.0, x = b;
    for (uint64_t k = uint64_t(n); k; k >>= 1) {
        if (k & 1) r = r * x;
        if (k >> 1) x = x * x;
    }
    return r;
}

// The scalars of update `step` at rate `lr`, as adamw_step_impl forms them: in fp64, each rounded
// to fp32 once; b^step by pow_chain.  The subtraction, the division and sqrt are IEEE-exact on
// the host and on the device (fp64 division and sqrt are correctly rounded there).
__host__ __device__ inline AdamwScalars adamw_sched_scalars(int64_t step, double lr, double beta1, double beta2,
                                                            double eps, double weight_decay, double alpha) {
    const double bc1 = 1.0 - pow_chain(beta1, step), bc2 = 1.0 - pow_chain(beta2, step);
    AdamwScalars s;
    s.decay = float(1.0 - lr * weight_decay);
    s.w1 = float(1.0 - beta1);
    s.b2 = float(beta2);
    s.w2 = float(1.0 - beta2);
    s.neg_step = float(-(lr / bc1));
    s.sqrt_bc2 = float(sqrt(bc2));
    s.eps = float(eps);
    s.alpha = float(alpha);
    s.beta = float(1.0 - alpha);
    return s;
}

struct AdvanceArgs {
    trlx_adamw_sched* sched;
    const double* lr_table;
    int64_t n_lr, sync_every;
    const trlx_grad_norm_record* rec;  // NULL: none
    int skip_nonfinite;
    double beta1, beta2, eps, weight_decay, alpha;
};

// One wave, one lane at work: the counter, the rate and the scalars of the update that the
// following k_adamw launches of this stream apply.
__global__ __launch_bounds__(kWave) void k_adamw_advance(AdvanceArgs a) {
    if (threadIdx.x != 0) return;
    trlx_adamw_sched* sc = a.sched;
    if (a.skip_nonfinite && a.rec && a.rec->nonfinite) {
        sc->apply = 0;
        sc->sync = 0;
        sc->skipped = sc->skipped + 1;
        return;
    }
    const int64_t step = sc->step + 1;
    const int64_t at = (step < a.n_lr ? step : a.n_lr) - 1;
    const double lr = a.lr_table[at < 0 ? 0 : at];  // a counter loaded below 0 still reads inside the table
    const AdamwScalars s = adamw_sched_scalars(step, lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.alpha);
    sc->step = step;
    sc->apply = 1;
    sc->sync = (a.sync_every > 0 && step % a.sync_every == 0) ? 1 : 0;
    sc->decay = s.decay;
    sc->w1 = s.w1;
    sc->b2 = s.b2;
    sc->w2 = s.w2;
    sc->neg_step = s.neg_step;
    sc->sqrt_bc2 = s.sqrt_bc2;
    sc->eps = s.eps;
    sc->alpha = s.alpha;
    sc->beta = s.beta;
    sc->pad = 0.f;
    sc->lr = lr;
}

// ------------------------------------------------------------------ global gradient norm
constexpr int kFinishThreads = 1024;

struct GradEntry {
    void* g;
    int64_t n;
    int dtype;  // TRLX_F32 / TRLX_BF16, per entry
};
struct GradTable {
    GradEntry e[TRLX_ADAMW_MAX_TENSORS];
    int blk0[TRLX_ADAMW_MAX_TENSORS + 1];  // first workgroup of each entry; [count] = the grid
    int count;
};

// [head | nvec 16-B vectors | tail] of one gradient, head and tail shorter than a vector; a
// workgroup takes TRLX_ADAMW_CHUNK elements' worth of vectors, workgroup 0 the head and tail too.
struct GradSplit {
    int64_t head, nvec, tail0, blocks;
    __host__ __device__ GradSplit(const GradEntry& e) {
        const int es = e.dtype == TRLX_BF16 ? 2 : 4, epv = 16 / es;
        head = int64_t(((16u - unsigned(reinterpret_cast<uintptr_t>(e.g) & 15u)) & 15u) / unsigned(es));
        if (head > e.n) head = e.n;
        nvec = (e.n - head) / epv;
        tail0 = head + nvec * epv;
        blocks = (nvec + TRLX_ADAMW_CHUNK / epv - 1) / (TRLX_ADAMW_CHUNK / epv);
        if (blocks < 1) blocks = 1;
    }
};

__device__ __forceinline__ int grad_entry_of_block(const GradTable& t) {
    int i = 0;
    while (i + 1 < t.count && int(blockIdx.x) >= t.blk0[i + 1]) ++i;  // block-uniform
    return i;
}

// This thread's share of Σ g² of chunk j: every element widened to fp64 before it is squared
// (1e20² is finite there), four chains per thread joined in a fixed order.
template <class GT>
__device__ __forceinline__ double grad_sumsq_chunk(const GradEntry& e, int64_t j, int tid) {
    typedef typename GT::elem_t GE;
    constexpr int kVecs = TRLX_ADAMW_CHUNK / GT::kEPV;  // vectors per workgroup
    const GradSplit sp(e);
    const vec4u* body = reinterpret_cast<const vec4u*>(static_cast<const GE*>(e.g) + sp.head);
    const int64_t v1 = min(sp.nvec, (j + 1) * kVecs);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int64_t q = j * kVecs + tid; q < v1; q += kAdamwThreads) {
        float f[GT::kEPV];
        GT::unpack(ld_stream(body + q), f);
#pragma unroll
        for (int k = 0; k < GT::kEPV; ++k) {
            const double d = double(f[k]);
            acc[k & 3] += d * d;
        }
    }
    if (j == 0) {  // the head and tail elements, fewer than a vector each
        int64_t k = -1;
        if (tid < sp.head) k = tid;
        else if (tid - sp.head < e.n - sp.tail0) k = sp.tail0 + (tid - sp.head);
        if (k >= 0) {
            const double d = double(GT::load1(e.g, k));
            acc[0] += d * d;
        }
    }
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ __launch_bounds__(kAdamwThreads) void k_grad_sumsq(GradTable t, double* partials) {
    __shared__ double sh[kAdamwThreads / kWave];
    const int i = grad_entry_of_block(t);
    const int64_t j = int(blockIdx.x) - t.blk0[i];
    const GradEntry e = t.e[i];
    const double mine = e.dtype == TRLX_BF16 ? grad_sumsq_chunk<BF16T>(e, j, threadIdx.x)
                                             : grad_sumsq_chunk<F32T>(e, j, threadIdx.x);
    const double s = block_sum_d(mine, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// All partials of all launches in one fixed order -> the record.  max_norm = +inf: the norm only.
__global__ __launch_bounds__(kFinishThreads) void k_grad_norm_finish(const double* partials, int n, float max_norm,
                                                                     trlx_grad_norm_record* rec) {
    __shared__ double sh[kFinishThreads / kWave];
    const double sumsq = reduce_records<1>(partials, n, sh);
    if (threadIdx.x != 0) return;
    const float norm = float(sqrt(sumsq));
    float coef = 1.f;
    if (max_norm != INFINITY) {
        // torch: max_norm / (norm + 1e-6) is (norm + 1e-6).reciprocal() * max_norm, then clamp(max=1)
        coef = mul_rn(__fdiv_rn(1.f, add_rn(norm, 1e-6f)), max_norm);
        if (coef > 1.f) coef = 1.f;  // a NaN stays
    }
    rec->norm = norm;
    rec->coef = coef;
    rec->nonfinite = isfinite(norm) ? 0 : 1;
    rec->pad = 0;
    rec->sumsq = sumsq;
    rec->reserved = 0;
}

// g <- g·coef in place, coef and the product each rounded to g's dtype: the stand-alone clip_grad_norm_.
template <class GT>
__device__ __forceinline__ void grad_scale_chunk(const GradEntry& e, int64_t j, int tid, float record_coef) {
    typedef typename GT::elem_t GE;
    const float coef = as_stored<GT>(record_coef);  // in g's dtype, as torch's g.mul_(coef) takes it
    constexpr int kVecs = TRLX_ADAMW_CHUNK / GT::kEPV;
    const GradSplit sp(e);
    vec4u* body = reinterpret_cast<vec4u*>(static_cast<GE*>(e.g) + sp.head);
    const int64_t v1 = min(sp.nvec, (j + 1) * kVecs);
#pragma unroll 4
    for (int64_t q = j * kVecs + tid; q < v1; q += kAdamwThreads) {
        float f[GT::kEPV];
        GT::unpack(body[q], f);
#pragma unroll
        for (int k = 0; k < GT::kEPV; ++k) f[k] = mul_rn(f[k], coef);
        body[q] = GT::pack(f);
    }
    if (j == 0) {
        int64_t k = -1;
        if (tid < sp.head) k = tid;
        else if (tid - sp.head < e.n - sp.tail0) k = sp.tail0 + (tid - sp.head);
        if (k >= 0) GT::store1(e.g, k, mul_rn(GT::load1(e.g, k), coef));
    }
}

__global__ __launch_bounds__(kAdamwThreads) void k_grad_scale(GradTable t, const trlx_grad_norm_record* rec) {
    const int i = grad_entry_of_block(t);
    const int64_t j = int(blockIdx.x) - t.blk0[i];
    const GradEntry e = t.e[i];
    const float coef = rec->coef;
    if (e.dtype == TRLX_BF16) grad_scale_chunk<BF16T>(e, j, threadIdx.x, coef);
    else grad_scale_chunk<F32T>(e, j, threadIdx.x, coef);
}

}  // namespace trlx

using namespace trlx;

static int adamw_launch(const AdamwTable& t, int p_dtype, int g_dtype, int s_dtype, const trlx_grad_norm_record* rec,
                        const trlx_adamw_sched* sched, hipStream_t stream) {
    const dim3 grid{unsigned(t.blk0[t.count])}, block(kAdamwThreads);
#define TRLX_ADAMW_LAUNCH_1(PT, GT, ST, CLIP, DEV) \
    hipLaunchKernelGGL((k_adamw<PT, GT, ST, CLIP, DEV>), grid, block, 0, stream, t, rec, sched)
#define TRLX_ADAMW_LAUNCH(PT, GT, ST)                                      \
    do {                                                                   \
        if (rec && sched) TRLX_ADAMW_LAUNCH_1(PT, GT, ST, true, true);     \
        else if (rec) TRLX_ADAMW_LAUNCH_1(PT, GT, ST, true, false);        \
        else if (sched) TRLX_ADAMW_LAUNCH_1(PT, GT, ST, false, true);      \
        else TRLX_ADAMW_LAUNCH_1(PT, GT, ST, false, false);                \
    } while (0)
    if (s_dtype == TRLX_BF16) TRLX_ADAMW_LAUNCH(BF16T, BF16T, BF16T);  // the caller checked p and g
    else if (p_dtype == TRLX_BF16 && g_dtype == TRLX_BF16) TRLX_ADAMW_LAUNCH(BF16T, BF16T, F32T);
    else if (p_dtype == TRLX_BF16) TRLX_ADAMW_LAUNCH(BF16T, F32T, F32T);
    else if (g_dtype == TRLX_BF16) TRLX_ADAMW_LAUNCH(F32T, BF16T, F32T);
    else TRLX_ADAMW_LAUNCH(F32T, F32T, F32T);
#undef TRLX_ADAMW_LAUNCH
#undef TRLX_ADAMW_LAUNCH_1
    return check_launch("k_adamw");
}

static AdamwEntry adamw_entry(const trlx_adamw_args& a, int64_t i) {
    AdamwEntry e;
    e.p = a.p[i];
    e.g = a.g[i];
    e.m = a.m[i];
    e.v = a.v[i];
    e.master = a.master ? static_cast<float*>(a.master[i]) : nullptr;
    e.target = a.target ? a.target[i] : nullptr;
    e.n = a.numel[i];
    return e;
}

static bool disjoint(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) {
    return a + a_bytes <= b || b + b_bytes <= a;
}

// rec: NULL for the plain step, the clip record (already checked non-NULL and aligned) otherwise.
// sched: NULL for the by-value scalars, the schedule record (checked likewise) otherwise: the
// scalar fields of args are then neither read nor validated.  s_dtype: the dtype of m and v.
static int adamw_step_impl(const trlx_adamw_args* args, int s_dtype, const trlx_grad_norm_record* rec,
                           const trlx_adamw_sched* sched, void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_adamw_args");
    const trlx_adamw_args& a = *args;
    TRLX_REQUIRE(s_dtype == TRLX_F32 || s_dtype == TRLX_BF16, TRLX_ERR_DTYPE, "adamw state dtype %d", s_dtype);
    TRLX_REQUIRE(a.p_dtype == TRLX_F32 || a.p_dtype == TRLX_BF16, TRLX_ERR_DTYPE, "adamw parameter dtype %d", a.p_dtype);
    TRLX_REQUIRE(a.g_dtype == TRLX_F32 || a.g_dtype == TRLX_BF16, TRLX_ERR_DTYPE, "adamw gradient dtype %d", a.g_dtype);
    TRLX_REQUIRE(s_dtype != TRLX_BF16 || (a.p_dtype == TRLX_BF16 && a.g_dtype == TRLX_BF16), TRLX_ERR_DTYPE,
                 "adamw: a bf16 state takes bf16 parameters and gradients (p_dtype %d, g_dtype %d)", a.p_dtype,
                 a.g_dtype);
    TRLX_REQUIRE(a.count >= 0 && (a.count == 0 || (a.p && a.g && a.m && a.v && a.numel)), TRLX_ERR_ARG,
                 "bad adamw tensor list");
    TRLX_REQUIRE(sched || a.step >= 1, TRLX_ERR_ARG, "adamw step %lld (the first update is step 1)", (long long)a.step);
    TRLX_REQUIRE(sched || (a.lr == a.lr && a.beta1 == a.beta1 && a.beta2 == a.beta2 && a.eps == a.eps &&
                           a.weight_decay == a.weight_decay),
                 TRLX_ERR_ARG, "adamw: a NaN hyper-parameter");
    TRLX_REQUIRE(!(sched && rec) || disjoint(reinterpret_cast<uintptr_t>(sched), sizeof(*sched),
                                             reinterpret_cast<uintptr_t>(rec), sizeof(*rec)),
                 TRLX_ERR_ARG, "adamw: the schedule record overlaps the clip record");
    // the table the record's advance reads, named so that the step can keep its tensors off it
    const uintptr_t lt = sched ? reinterpret_cast<uintptr_t>(a.lr_table) : 0;
    const uintptr_t lt_bytes = lt ? uintptr_t(a.n_lr) * 8u : 0;
    if (lt) {
        TRLX_REQUIRE((lt & 7u) == 0, TRLX_ERR_ARG, "the lr_table is not aligned to 8 bytes");
        TRLX_REQUIRE(a.n_lr >= 1 && a.n_lr <= (int64_t(1) << 40), TRLX_ERR_ARG,
                     "adamw: n_lr %lld (at least one rate)", (long long)a.n_lr);
        TRLX_REQUIRE(disjoint(lt, lt_bytes, reinterpret_cast<uintptr_t>(sched), sizeof(*sched)), TRLX_ERR_ARG,
                     "adamw: the schedule record overlaps the lr_table");
        TRLX_REQUIRE(!rec || disjoint(lt, lt_bytes, reinterpret_cast<uintptr_t>(rec), sizeof(*rec)), TRLX_ERR_ARG,
                     "adamw: the lr_table overlaps the clip record");
    }
    const int p_es = a.p_dtype == TRLX_BF16 ? 2 : 4, g_es = a.g_dtype == TRLX_BF16 ? 2 : 4;
    const int s_es = s_dtype == TRLX_BF16 ? 2 : 4;
    static const char* const kNames[6] = {"p", "g", "m", "v", "master", "target"};
    for (int64_t i = 0; i < a.count; ++i) {  // validate everything before the first launch
        const AdamwEntry e = adamw_entry(a, i);
        TRLX_REQUIRE(e.n >= 0, TRLX_ERR_SHAPE, "adamw tensor %lld: numel %lld", (long long)i, (long long)e.n);
        if (e.n == 0) continue;
        TRLX_REQUIRE(e.p && e.g && e.m && e.v, TRLX_ERR_ARG, "adamw tensor %lld: NULL pointer", (long long)i);
        TRLX_REQUIRE(!(e.master && a.p_dtype != TRLX_BF16), TRLX_ERR_ARG,
                     "adamw tensor %lld: a master is for a bf16 parameter", (long long)i);
        TRLX_REQUIRE(!(e.master && s_dtype == TRLX_BF16), TRLX_ERR_ARG,
                     "adamw tensor %lld: a bf16 state takes no master", (long long)i);
        TRLX_REQUIRE(!e.target || sched || a.alpha == a.alpha, TRLX_ERR_ARG, "adamw: alpha is NaN");
        TRLX_REQUIRE(e.n <= int64_t(TRLX_ADAMW_CHUNK) * kAdamwMaxGrid, TRLX_ERR_SHAPE,
                     "adamw tensor %lld too large (%lld elements)", (long long)i, (long long)e.n);
        const uintptr_t ptr[6] = {reinterpret_cast<uintptr_t>(e.p),      reinterpret_cast<uintptr_t>(e.g),
                                  reinterpret_cast<uintptr_t>(e.m),      reinterpret_cast<uintptr_t>(e.v),
                                  reinterpret_cast<uintptr_t>(e.master), reinterpret_cast<uintptr_t>(e.target)};
        const int es[6] = {p_es, g_es, s_es, s_es, 4, p_es};
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
        for (int x = 0; rec && x < 6; ++x)
            TRLX_REQUIRE(!ptr[x] || disjoint(reinterpret_cast<uintptr_t>(rec), sizeof(*rec), ptr[x],
                                             uintptr_t(e.n) * uintptr_t(es[x])),
                         TRLX_ERR_ARG, "adamw tensor %lld: the clip record overlaps %s", (long long)i, kNames[x]);
        for (int x = 0; sched && x < 6; ++x)
            TRLX_REQUIRE(!ptr[x] || disjoint(reinterpret_cast<uintptr_t>(sched), sizeof(*sched), ptr[x],
                                             uintptr_t(e.n) * uintptr_t(es[x])),
                         TRLX_ERR_ARG, "adamw tensor %lld: the schedule record overlaps %s", (long long)i, kNames[x]);
        for (int x = 0; lt && x < 6; ++x)
            TRLX_REQUIRE(!ptr[x] || disjoint(lt, lt_bytes, ptr[x], uintptr_t(e.n) * uintptr_t(es[x])), TRLX_ERR_ARG,
                         "adamw tensor %lld: the lr_table overlaps %s", (long long)i, kNames[x]);
    }
    // the scalars, formed in double as torch forms them, rounded to fp32 once (with a schedule
    // record the kernel reads its own: these are formed from ignored fields and never used)
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
        const int64_t blocks = AdamwSplit(e, p_es, g_es, s_es).blocks;
        if (t.count == TRLX_ADAMW_MAX_TENSORS || t.blk0[t.count] + blocks > kAdamwMaxGrid) {
            const int rc = adamw_launch(t, a.p_dtype, a.g_dtype, s_dtype, rec, sched, (hipStream_t)stream);
            if (rc) return rc;
            t.count = 0;
        }
        t.e[t.count] = e;
        t.blk0[t.count + 1] = int(t.blk0[t.count] + blocks);
        ++t.count;
    }
    return t.count ? adamw_launch(t, a.p_dtype, a.g_dtype, s_dtype, rec, sched, (hipStream_t)stream) : TRLX_OK;
}

extern "C" int trlx_adamw_step(const trlx_adamw_args* args, void* stream) {
    return adamw_step_impl(args, TRLX_F32, nullptr, nullptr, stream);
}

static int check_record(const void* record) {
    TRLX_REQUIRE(record, TRLX_ERR_ARG, "NULL grad-norm record");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(record) & 7u) == 0, TRLX_ERR_ARG,
                 "the grad-norm record is not aligned to 8 bytes");
    return TRLX_OK;
}

extern "C" int trlx_adamw_step_clipped(const trlx_adamw_args* args, const void* record, void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_adamw_args");
    const int rc = check_record(record);
    if (rc) return rc;
    return adamw_step_impl(args, TRLX_F32, static_cast<const trlx_grad_norm_record*>(record), nullptr, stream);
}

static int check_sched(const void* sched) {
    TRLX_REQUIRE(sched, TRLX_ERR_ARG, "NULL schedule record");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(sched) & 7u) == 0, TRLX_ERR_ARG,
                 "the schedule record is not aligned to 8 bytes");
    return TRLX_OK;
}

extern "C" int trlx_adamw_step_dev(const trlx_adamw_args* args, const void* sched, void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_adamw_args");
    const int rc = check_sched(sched);
    if (rc) return rc;
    return adamw_step_impl(args, TRLX_F32, nullptr, static_cast<const trlx_adamw_sched*>(sched), stream);
}

extern "C" int trlx_adamw_step_clipped_dev(const trlx_adamw_args* args, const void* grad_record, const void* sched,
                                           void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_adamw_args");
    int rc = check_record(grad_record);
    if (rc) return rc;
    rc = check_sched(sched);
    if (rc) return rc;
    return adamw_step_impl(args, TRLX_F32, static_cast<const trlx_grad_norm_record*>(grad_record),
                           static_cast<const trlx_adamw_sched*>(sched), stream);
}

// Every launch form with the dtype of m and v chosen by the caller: grad_record NULL = unclipped,
// sched NULL = the scalars of args.  TRLX_F32 is the four entries above.
extern "C" int trlx_adamw_step_ex(const trlx_adamw_args* args, int state_dtype, const void* grad_record,
                                  const void* sched, void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_adamw_args");
    int rc = grad_record ? check_record(grad_record) : TRLX_OK;
    if (rc) return rc;
    rc = sched ? check_sched(sched) : TRLX_OK;
    if (rc) return rc;
    return adamw_step_impl(args, state_dtype, static_cast<const trlx_grad_norm_record*>(grad_record),
                           static_cast<const trlx_adamw_sched*>(sched), stream);
}

extern "C" int trlx_adamw_sched_scalars_host(int64_t step, double lr, double beta1, double beta2, double eps,
                                             double weight_decay, double alpha, float* out) {
    TRLX_REQUIRE(out, TRLX_ERR_ARG, "NULL output of the schedule scalars");
    TRLX_REQUIRE(step >= 1, TRLX_ERR_ARG, "adamw step %lld (the first update is step 1)", (long long)step);
    const AdamwScalars s = adamw_sched_scalars(step, lr, beta1, beta2, eps, weight_decay, alpha);
    const float v[9] = {s.decay, s.w1, s.b2, s.w2, s.neg_step, s.sqrt_bc2, s.eps, s.alpha, s.beta};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
    return TRLX_OK;
}

extern "C" int trlx_adamw_advance(const trlx_adamw_advance_args* args, void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_adamw_advance_args");
    const trlx_adamw_advance_args& a = *args;
    int rc = check_sched(a.sched);
    if (rc) return rc;
    TRLX_REQUIRE(a.lr_table, TRLX_ERR_ARG, "NULL lr_table");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(a.lr_table) & 7u) == 0, TRLX_ERR_ARG,
                 "the lr_table is not aligned to 8 bytes");
    TRLX_REQUIRE(a.n_lr >= 1, TRLX_ERR_ARG, "adamw advance: n_lr %lld (at least one rate)", (long long)a.n_lr);
    TRLX_REQUIRE(a.n_lr <= (int64_t(1) << 40), TRLX_ERR_ARG, "adamw advance: n_lr %lld too large", (long long)a.n_lr);
    TRLX_REQUIRE(a.sync_every >= 0, TRLX_ERR_ARG, "adamw advance: sync_every %lld (0: never)", (long long)a.sync_every);
    TRLX_REQUIRE(a.beta1 == a.beta1 && a.beta2 == a.beta2 && a.eps == a.eps && a.weight_decay == a.weight_decay &&
                     a.alpha == a.alpha,
                 TRLX_ERR_ARG, "adamw advance: a NaN hyper-parameter");
    if (a.grad_record) {
        rc = check_record(a.grad_record);
        if (rc) return rc;
    }
    const uintptr_t sc = reinterpret_cast<uintptr_t>(a.sched), lt = reinterpret_cast<uintptr_t>(a.lr_table),
                    gr = reinterpret_cast<uintptr_t>(a.grad_record), lt_bytes = uintptr_t(a.n_lr) * 8u;
    TRLX_REQUIRE(disjoint(sc, sizeof(trlx_adamw_sched), lt, lt_bytes), TRLX_ERR_ARG,
                 "adamw advance: the schedule record overlaps the lr_table");
    TRLX_REQUIRE(!gr || disjoint(sc, sizeof(trlx_adamw_sched), gr, sizeof(trlx_grad_norm_record)), TRLX_ERR_ARG,
                 "adamw advance: the schedule record overlaps the grad-norm record");
    TRLX_REQUIRE(!gr || disjoint(lt, lt_bytes, gr, sizeof(trlx_grad_norm_record)), TRLX_ERR_ARG,
                 "adamw advance: the lr_table overlaps the grad-norm record");
    AdvanceArgs k;
    k.sched = static_cast<trlx_adamw_sched*>(a.sched);
    k.lr_table = static_cast<const double*>(a.lr_table);
    k.n_lr = a.n_lr;
    k.sync_every = a.sync_every;
    k.rec = static_cast<const trlx_grad_norm_record*>(a.grad_record);
    k.skip_nonfinite = a.skip_nonfinite;
    k.beta1 = a.beta1, k.beta2 = a.beta2, k.eps = a.eps, k.weight_decay = a.weight_decay, k.alpha = a.alpha;
    hipLaunchKernelGGL(k_adamw_advance, dim3(1), dim3(kWave), 0, (hipStream_t)stream, k);
    return check_launch("k_adamw_advance");
}

// workgroups of k_grad_sumsq for n elements, whatever the dtype and the alignment: at most
// ceil(n / CHUNK) (a head only shortens the body), at least one
static int64_t grad_blocks_bound(int64_t n) {
    return n == 0 ? 0 : (n + TRLX_ADAMW_CHUNK - 1) / TRLX_ADAMW_CHUNK;
}

extern "C" int64_t trlx_grad_norm_workspace_bytes(const int64_t* numel, int64_t count) {
    if (count < 0 || (count > 0 && !numel)) return -1;
    int64_t blocks = 0;
    for (int64_t i = 0; i < count; ++i) {
        if (numel[i] < 0) return -1;
        blocks += grad_blocks_bound(numel[i]);
    }
    return 8 * (blocks < 1 ? 1 : blocks);
}

static GradEntry grad_entry(const trlx_grad_norm_args& a, int64_t i) {
    GradEntry e;
    e.g = const_cast<void*>(a.g[i]);
    e.n = a.numel[i];
    e.dtype = a.g_dtype[i];
    return e;
}

// One launch per table of up to TRLX_ADAMW_MAX_TENSORS live tensors: the sumsq launches write
// their partials one after the other (*n_partials counts them), the scale launches read `rec`.
static int grad_launches(const trlx_grad_norm_args& a, bool scale, double* partials, int64_t* n_partials,
                         const trlx_grad_norm_record* rec, hipStream_t stream) {
    GradTable t;
    t.count = 0;
    t.blk0[0] = 0;
    int64_t done = 0;
    for (int64_t i = 0; i <= a.count; ++i) {
        GradEntry e{};
        int64_t blocks = 0;
        if (i < a.count) {
            e = grad_entry(a, i);
            if (e.n == 0) continue;  // zero-length tensors are skipped
            blocks = GradSplit(e).blocks;
        }
        if (t.count && (i == a.count || t.count == TRLX_ADAMW_MAX_TENSORS || t.blk0[t.count] + blocks > kAdamwMaxGrid)) {
            const dim3 grid{unsigned(t.blk0[t.count])}, block(kAdamwThreads);
            if (scale) hipLaunchKernelGGL(k_grad_scale, grid, block, 0, stream, t, rec);
            else hipLaunchKernelGGL(k_grad_sumsq, grid, block, 0, stream, t, partials + done);
            const int rc = check_launch(scale ? "k_grad_scale" : "k_grad_sumsq");
            if (rc) return rc;
            done += t.blk0[t.count];
            t.count = 0;
        }
        if (i == a.count) break;
        t.e[t.count] = e;
        t.blk0[t.count + 1] = int(t.blk0[t.count] + blocks);
        ++t.count;
    }
    if (n_partials) *n_partials = done;
    return TRLX_OK;
}

extern "C" int trlx_grad_norm(const trlx_grad_norm_args* args, void* stream) {
    TRLX_REQUIRE(args, TRLX_ERR_ARG, "NULL trlx_grad_norm_args");
    const trlx_grad_norm_args& a = *args;
    TRLX_REQUIRE(a.count >= 0 && (a.count == 0 || (a.g && a.g_dtype && a.numel)), TRLX_ERR_ARG,
                 "bad grad-norm tensor list");
    TRLX_REQUIRE(a.max_norm == a.max_norm && a.max_norm >= 0.0, TRLX_ERR_ARG,
                 "grad-norm max_norm %g (must be >= 0, +inf records the norm only)", a.max_norm);
    TRLX_REQUIRE(a.scale_in_place >= 0 && a.scale_in_place <= 2, TRLX_ERR_ARG, "grad-norm scale_in_place %d",
                 a.scale_in_place);
    const int rc = check_record(a.record);
    if (rc) return rc;
    TRLX_REQUIRE(a.workspace, TRLX_ERR_ARG, "NULL grad-norm workspace");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(a.workspace) & 7u) == 0, TRLX_ERR_ARG,
                 "the grad-norm workspace is not aligned to 8 bytes");
    const uintptr_t rec = reinterpret_cast<uintptr_t>(a.record), ws = reinterpret_cast<uintptr_t>(a.workspace);
    int64_t bound = 0;
    for (int64_t i = 0; i < a.count; ++i) {  // validate everything before the first launch
        const GradEntry e = grad_entry(a, i);
        TRLX_REQUIRE(e.n >= 0, TRLX_ERR_SHAPE, "grad-norm tensor %lld: numel %lld", (long long)i, (long long)e.n);
        if (e.n == 0) continue;
        TRLX_REQUIRE(e.dtype == TRLX_F32 || e.dtype == TRLX_BF16, TRLX_ERR_DTYPE, "grad-norm tensor %lld: dtype %d",
                     (long long)i, e.dtype);
        TRLX_REQUIRE(e.g, TRLX_ERR_ARG, "grad-norm tensor %lld: NULL pointer", (long long)i);
        TRLX_REQUIRE(e.n <= int64_t(TRLX_ADAMW_CHUNK) * kAdamwMaxGrid, TRLX_ERR_SHAPE,
                     "grad-norm tensor %lld too large (%lld elements)", (long long)i, (long long)e.n);
        const int es = e.dtype == TRLX_BF16 ? 2 : 4;
        const uintptr_t g = reinterpret_cast<uintptr_t>(e.g), bytes = uintptr_t(e.n) * uintptr_t(es);
        TRLX_REQUIRE((g & uintptr_t(es - 1)) == 0, TRLX_ERR_ARG,
                     "grad-norm tensor %lld: g not aligned to the element size", (long long)i);
        bound += grad_blocks_bound(e.n);
        TRLX_REQUIRE(bound < (int64_t(1) << 31), TRLX_ERR_SHAPE, "grad-norm: too many elements for one record");
        TRLX_REQUIRE(disjoint(rec, sizeof(trlx_grad_norm_record), g, bytes), TRLX_ERR_ARG,
                     "grad-norm tensor %lld: the record overlaps g", (long long)i);
        TRLX_REQUIRE(a.workspace_bytes <= 0 || disjoint(ws, uintptr_t(a.workspace_bytes), g, bytes), TRLX_ERR_ARG,
                     "grad-norm tensor %lld: the workspace overlaps g", (long long)i);
    }
    const int64_t need = 8 * (bound < 1 ? 1 : bound);
    TRLX_REQUIRE(a.workspace_bytes >= need, TRLX_ERR_ARG, "grad-norm workspace of %lld bytes, %lld needed",
                 (long long)a.workspace_bytes, (long long)need);
    TRLX_REQUIRE(disjoint(rec, sizeof(trlx_grad_norm_record), ws, uintptr_t(a.workspace_bytes)), TRLX_ERR_ARG,
                 "grad-norm: the record overlaps the workspace");
    trlx_grad_norm_record* record = static_cast<trlx_grad_norm_record*>(a.record);
    if (a.scale_in_place != 2) {
        int64_t n_partials = 0;
        int rc2 = grad_launches(a, false, static_cast<double*>(a.workspace), &n_partials, nullptr, (hipStream_t)stream);
        if (rc2) return rc2;
        hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(kFinishThreads), 0, (hipStream_t)stream,
                           static_cast<const double*>(a.workspace), int(n_partials), float(a.max_norm), record);
        rc2 = check_launch("k_grad_norm_finish");
        if (rc2) return rc2;
    }
    return a.scale_in_place ? grad_launches(a, true, nullptr, nullptr, record, (hipStream_t)stream) : TRLX_OK;
}
