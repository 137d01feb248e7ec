// T5 decode-step attention over a device KV cache: one query token per (batch row, head), one
// launch, one workgroup per (batch row, head).  See trlx_t5_decode_attn in trlx_t5_amd.h.
//
// Layout.  A key row is d_kv elements; each lane takes one 16-byte vector of it, so LPR = d_kv /
// (elements per vector) lanes cover a row and one wave-wide load covers KPW = 64 / LPR rows
// (bf16 d_kv 64: 8 lanes a row, 8 rows a load).  The LPR lanes of a row form a group.  A group
// holds its slice of q in fp32 registers, reduces its partial dot products with a butterfly inside
// the group and keeps its own online-softmax state (running max, running sum, its slice of P·V in
// fp32): no cross-group traffic inside the loop.  The 4 waves x KPW groups walk the cached columns
// round-robin, two columns per group in flight.  At the end every group parks its state in LDS and
// d_kv / 2 threads merge the groups in a fixed order, divide and round once.
//
// Self-attention: group 0 holds k_new / v_new of this (row, head) in registers, stores them to
// column t of the cache and attends to them FROM THE REGISTERS; the loop reads columns 0..t-1
// only, so nothing written by this launch is read by it and columns above t are never touched.
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace trlx {

constexpr int kT5Threads = 256;
constexpr int kT5Waves = kT5Threads / kWave;

enum { kT5Self = 0, kT5Cross = 1, kT5CrossMasked = 2 };

struct T5AttnArgs {
    const void* q;
    const void* k_new;
    const void* v_new;
    void* k;
    void* v;
    const float* bias;      // [nH, max_len] or NULL
    const int64_t* mask;    // [B, max_len] or NULL
    void* out;
    int64_t ldq, ldk, ldv;
    int nH, max_len, t;
};

// The device-clock step (trlx_t5_decode_attn_dev): t comes from the decode clock, a.t is not read.
struct T5AttnDevArgs {
    T5AttnArgs a;
    const int64_t* clock;
};
// The live-row step (trlx_t5_decode_attn_live): live[b] == 0 skips row b; clock as above or NULL.
struct T5AttnLiveArgs {
    T5AttnArgs a;
    const int64_t* clock;
    const int64_t* live;    // [B]
};
__device__ __forceinline__ const T5AttnArgs& t5_args(const T5AttnArgs& a) { return a; }
__device__ __forceinline__ const T5AttnArgs& t5_args(const T5AttnDevArgs& a) { return a.a; }
__device__ __forceinline__ const T5AttnArgs& t5_args(const T5AttnLiveArgs& a) { return a.a; }

// zeros to out[b, h, :]: what a dead step and a skipped row store
template <class E, int DKV>
__device__ __forceinline__ void t5_zero_out(void* out, int bh) {
    if (threadIdx.x < DKV / 2) {
        const int64_t o = int64_t(bh) * DKV + 2 * threadIdx.x;
        if (sizeof(E) == 2) {
            *reinterpret_cast<uint32_t*>(static_cast<uint16_t*>(out) + o) = 0u;
        } else {
            float2 z;
            z.x = 0.f;
            z.y = 0.f;
            *reinterpret_cast<float2*>(static_cast<float*>(out) + o) = z;
        }
    }
}

template <class DT>
__device__ __forceinline__ vec4u t5_ld(const typename DT::elem_t* p) {
    return *reinterpret_cast<const vec4u*>(p);
}

// MODE: kT5Self (append + bias), kT5Cross (no mask), kT5CrossMasked (key_mask given)
// DEVT (kT5Self only): t and the capacity T are loaded from the decode clock, once, at the top of
// the workgroup (uniform loads from a kernel-argument pointer).  A step with t outside
// [0, min(T, max_len)) is dead: zeros to out[b, h, :] and out, before any address is formed from t
// and before any barrier; the exit is uniform.  DEVT = false compiles to the kernel without it.
// LIVE: the workgroup loads live[b] first, one uniform load; a row with live[b] == 0 gets zeros in
// out[b, h, :] and the workgroup leaves, before any barrier and before any address is formed into
// q, k_new, v_new, the cache, the mask or the bias: column t of a skipped row stays unwritten.  A
// row with live[b] != 0 runs the code below unchanged.  LIVE = false compiles to the kernel without it.
template <class DT, int DKV, int MODE, bool DEVT = false, bool LIVE = false>
__global__ __launch_bounds__(kT5Threads) void k_t5_decode_attn(
    const std::conditional_t<LIVE, T5AttnLiveArgs, std::conditional_t<DEVT, T5AttnDevArgs, T5AttnArgs>> args) {
    static_assert(!DEVT || MODE == kT5Self, "only the self-attention reads t");
    const T5AttnArgs& a = t5_args(args);
    typedef typename DT::elem_t E;
    constexpr int EPV = DT::kEPV;
    constexpr int LPR = DKV / EPV;             // lanes per key row
    constexpr int KPW = kWave / LPR;           // key rows per wave-wide load
    constexpr int NG = kT5Waves * KPW;         // groups per workgroup
    static_assert(DKV % EPV == 0 && kWave % LPR == 0 && LPR >= 2, "row geometry");
    __shared__ float s_acc[NG * DKV];
    __shared__ float s_m[NG];
    __shared__ float s_l[NG];

    const int bh = blockIdx.x;
    const int b = bh / a.nH, h = bh - b * a.nH;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int sl = lane % LPR;                 // this lane's vector of the row
    const int gg = wave * KPW + lane / LPR;    // group id in the workgroup
    const int col = h * DKV + sl * EPV;
    if constexpr (LIVE) {
        if (args.live[b] == 0) {   // block-uniform
            t5_zero_out<E, DKV>(a.out, bh);
            return;
        }
    }
    [[maybe_unused]] int t_clock = 0;
    if constexpr (DEVT) {
        const int64_t tc = args.clock[TRLX_CLOCK_T], cap = args.clock[TRLX_CLOCK_CAP];
        const int64_t lim = cap < int64_t(a.max_len) ? cap : int64_t(a.max_len);
        if (tc < 0 || tc >= lim) {   // block-uniform
            t5_zero_out<E, DKV>(a.out, bh);
            return;
        }
        t_clock = int(tc);
    }
    const int t = DEVT ? t_clock : a.t;

    float qf[EPV];
    DT::unpack(t5_ld<DT>(static_cast<const E*>(a.q) + int64_t(b) * a.ldq + col), qf);
    vec4u kn = vec4u_make(0, 0, 0, 0), vn = kn;
    const bool owner = MODE == kT5Self && gg == 0;
    if (owner) {
        kn = t5_ld<DT>(static_cast<const E*>(a.k_new) + int64_t(b) * a.ldk + col);
        vn = t5_ld<DT>(static_cast<const E*>(a.v_new) + int64_t(b) * a.ldv + col);
    }
    const int64_t base = int64_t(bh) * a.max_len * DKV + sl * EPV;
    const E* K = static_cast<const E*>(a.k) + base;
    const E* V = static_cast<const E*>(a.v) + base;
    const float* bias = MODE == kT5Self && a.bias ? a.bias + int64_t(h) * a.max_len : nullptr;
    const int64_t* mask = MODE == kT5CrossMasked ? a.mask + int64_t(b) * a.max_len : nullptr;

    float m = -INFINITY, l = 0.f, acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.f;

    // one key: fp32 dot over the row (butterfly inside the group), the online max / sum, P·V
    auto step = [&](const vec4u& kv, const vec4u& vv, float bj) {
        float kf[EPV], vf[EPV];
        DT::unpack(kv, kf);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < EPV; ++e) s = fmaf(qf[e], kf[e], s);
#pragma unroll
        for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
        s += bj;
        const float mn = fmaxf(m, s);
        const float sc = expf(m - mn), p = expf(s - mn);
        l = fmaf(l, sc, p);
        DT::unpack(vv, vf);
#pragma unroll
        for (int e = 0; e < EPV; ++e) acc[e] = fmaf(acc[e], sc, p * vf[e]);
        m = mn;
    };

    const int n = MODE == kT5Self ? t : a.max_len;   // columns read from memory: [0, n)
#pragma unroll 1
    for (int j0 = gg; j0 < n; j0 += 2 * NG) {
        const int j1 = j0 + NG;
        bool live0 = true, live1 = j1 < n;
        if (MODE == kT5CrossMasked) {
            live0 = mask[j0] != 0;
            live1 = live1 && mask[j1] != 0;
        }
        vec4u k0 = vec4u_make(0, 0, 0, 0), v0 = k0, k1 = k0, v1 = k0;
        float b0 = 0.f, b1 = 0.f;
        if (live0) {
            k0 = t5_ld<DT>(K + int64_t(j0) * DKV);
            v0 = t5_ld<DT>(V + int64_t(j0) * DKV);
            if (bias) b0 = bias[t - j0];
        }
        if (live1) {
            k1 = t5_ld<DT>(K + int64_t(j1) * DKV);
            v1 = t5_ld<DT>(V + int64_t(j1) * DKV);
            if (bias) b1 = bias[t - j1];
        }
        if (live0) step(k0, v0, b0);
        if (live1) step(k1, v1, b1);
    }
    if (owner) {   // the new token: into column t of the cache, attended from the registers
        E* Kw = static_cast<E*>(a.k) + base + int64_t(t) * DKV;
        E* Vw = static_cast<E*>(a.v) + base + int64_t(t) * DKV;
        *reinterpret_cast<vec4u*>(Kw) = kn;
        *reinterpret_cast<vec4u*>(Vw) = vn;
        step(kn, vn, bias ? bias[0] : 0.f);
    }

    // merge: every group parks (m, l, its slice of P·V); d_kv / 2 threads combine them in group order
#pragma unroll
    for (int e = 0; e < EPV; ++e) s_acc[gg * DKV + sl * EPV + e] = acc[e];
    if (sl == 0) {
        s_m[gg] = m;
        s_l[gg] = l;
    }
    __syncthreads();
    if (threadIdx.x < DKV / 2) {
        const int d = 2 * threadIdx.x;
        float M = s_m[0];
        for (int g = 1; g < NG; ++g) M = fmaxf(M, s_m[g]);
        float L = 0.f, o0 = 0.f, o1 = 0.f;
        for (int g = 0; g < NG; ++g) {
            const float mg = s_m[g];
            if (mg == -INFINITY) continue;   // a group that saw no live key
            const float w = expf(mg - M);
            L = fmaf(s_l[g], w, L);
            o0 = fmaf(s_acc[g * DKV + d], w, o0);
            o1 = fmaf(s_acc[g * DKV + d + 1], w, o1);
        }
        // no live key at all (a fully masked row): zeros
        const bool any = L > 0.f || L != L;
        o0 = any ? o0 / L : 0.f;
        o1 = any ? o1 / L : 0.f;
        const int64_t o = int64_t(bh) * DKV + d;
        if (sizeof(E) == 2) {
            *reinterpret_cast<uint32_t*>(static_cast<uint16_t*>(a.out) + o) = pack_bf2(o0, o1);
        } else {
            float2 r;
            r.x = o0;
            r.y = o1;
            *reinterpret_cast<float2*>(static_cast<float*>(a.out) + o) = r;
        }
    }
}

typedef void (*t5_kernel_t)(const T5AttnArgs);
template <class DT, int DKV>
static t5_kernel_t t5_pick_mode(int mode) {
    return mode == kT5Self ? k_t5_decode_attn<DT, DKV, kT5Self>
           : mode == kT5Cross ? k_t5_decode_attn<DT, DKV, kT5Cross>
                              : k_t5_decode_attn<DT, DKV, kT5CrossMasked>;
}
static t5_kernel_t t5_pick(int dtype, int64_t d_kv, int mode) {
    if (dtype == TRLX_BF16) return d_kv == 64 ? t5_pick_mode<BF16T, 64>(mode) : t5_pick_mode<BF16T, 128>(mode);
    return d_kv == 64 ? t5_pick_mode<F32T, 64>(mode) : t5_pick_mode<F32T, 128>(mode);
}

static bool t5_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace trlx

using namespace trlx;

// The argument checks of both entries and the kernel's argument block.  dev: a->t is not read.
static int t5_decode_attn_prepare(const TrlxT5DecodeAttnArgs* a, bool dev, T5AttnArgs* args) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 decode attention: NULL arguments");
    TRLX_REQUIRE(a->dtype == TRLX_BF16 || a->dtype == TRLX_F32, TRLX_ERR_ARG,
                 "t5 decode attention: dtype %d (bf16 and fp32 only)", a->dtype);
    TRLX_REQUIRE(a->d_kv == 64 || a->d_kv == 128, TRLX_ERR_ARG, "t5 decode attention: d_kv %lld (64 and 128 only)",
                 (long long)a->d_kv);
    TRLX_REQUIRE(a->mode == TRLX_T5_ATTN_SELF || a->mode == TRLX_T5_ATTN_CROSS, TRLX_ERR_ARG,
                 "t5 decode attention: mode %d", a->mode);
    const bool self = a->mode == TRLX_T5_ATTN_SELF;
    TRLX_REQUIRE(a->B >= 1 && a->n_heads >= 1 && a->max_len >= 1 && a->B * a->n_heads <= 0x7fffffffLL &&
                     a->max_len <= 0x7fffffffLL / 128 && a->n_heads <= 0x7fffffffLL / 128,
                 TRLX_ERR_ARG, "t5 decode attention: B %lld, heads %lld, max_len %lld", (long long)a->B,
                 (long long)a->n_heads, (long long)a->max_len);
    TRLX_REQUIRE(a->q && a->k && a->v && a->out, TRLX_ERR_ARG, "t5 decode attention: NULL q / K / V / out");
    const int64_t inner = a->n_heads * a->d_kv;
    const int64_t epv = a->dtype == TRLX_BF16 ? 8 : 4;
    // a single row has no stride to speak of
    const int64_t ldq = a->B == 1 ? inner : a->ldq;
    TRLX_REQUIRE(ldq >= inner && ldq % epv == 0, TRLX_ERR_ARG,
                 "t5 decode attention: q row stride %lld (>= heads * d_kv = %lld, whole 16-byte vectors)",
                 (long long)ldq, (long long)inner);
    TRLX_REQUIRE(t5_aligned16(a->q) && t5_aligned16(a->k) && t5_aligned16(a->v) && t5_aligned16(a->out), TRLX_ERR_ARG,
                 "t5 decode attention: q, K, V and out must be 16-byte aligned");
    int64_t ldk = 0, ldv = 0;
    if (self) {
        TRLX_REQUIRE(dev || (a->t >= 0 && a->t < a->max_len), TRLX_ERR_ARG, "t5 decode attention: t %lld outside [0, max_len %lld)",
                     (long long)a->t, (long long)a->max_len);
        TRLX_REQUIRE(a->k_new && a->v_new, TRLX_ERR_ARG, "t5 decode attention: NULL k_new / v_new");
        ldk = a->B == 1 ? inner : a->ldk;
        ldv = a->B == 1 ? inner : a->ldv;
        TRLX_REQUIRE(ldk >= inner && ldk % epv == 0 && ldv >= inner && ldv % epv == 0, TRLX_ERR_ARG,
                     "t5 decode attention: k_new / v_new row strides %lld / %lld (>= heads * d_kv = %lld, whole "
                     "16-byte vectors)", (long long)ldk, (long long)ldv, (long long)inner);
        TRLX_REQUIRE(t5_aligned16(a->k_new) && t5_aligned16(a->v_new), TRLX_ERR_ARG,
                     "t5 decode attention: k_new and v_new must be 16-byte aligned");
        TRLX_REQUIRE(!a->key_mask, TRLX_ERR_ARG, "t5 decode attention: key_mask is for the cross-attention only");
        TRLX_REQUIRE(!a->bias_by_distance || (reinterpret_cast<uintptr_t>(a->bias_by_distance) & 3u) == 0, TRLX_ERR_ARG,
                     "t5 decode attention: bias_by_distance not aligned to 4 bytes");
    } else {
        TRLX_REQUIRE(!a->k_new && !a->v_new && !a->bias_by_distance, TRLX_ERR_ARG,
                     "t5 decode attention: k_new / v_new / bias_by_distance are for the self-attention only");
        TRLX_REQUIRE(!a->key_mask || (reinterpret_cast<uintptr_t>(a->key_mask) & 7u) == 0, TRLX_ERR_ARG,
                     "t5 decode attention: key_mask not aligned to 8 bytes");
    }
    T5AttnArgs k = {};
    k.q = a->q;
    k.k_new = a->k_new;
    k.v_new = a->v_new;
    k.k = a->k;
    k.v = a->v;
    k.bias = a->bias_by_distance;
    k.mask = a->key_mask;
    k.out = a->out;
    k.ldq = ldq;
    k.ldk = ldk;
    k.ldv = ldv;
    k.nH = int(a->n_heads);
    k.max_len = int(a->max_len);
    k.t = dev ? 0 : int(a->t);
    *args = k;
    return TRLX_OK;
}

extern "C" int trlx_t5_decode_attn(const TrlxT5DecodeAttnArgs* a, void* stream) {
    T5AttnArgs k;
    const int rc = t5_decode_attn_prepare(a, false, &k);
    if (rc) return rc;
    const int mode = a->mode == TRLX_T5_ATTN_SELF ? kT5Self : a->key_mask ? kT5CrossMasked : kT5Cross;
    hipLaunchKernelGGL(t5_pick(a->dtype, a->d_kv, mode), dim3(unsigned(a->B * a->n_heads)), dim3(kT5Threads), 0,
                       (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn");
}

typedef void (*t5_clock_kernel_t)(const T5AttnDevArgs);
static t5_clock_kernel_t t5_pick_clock(int dtype, int64_t d_kv) {
    if (dtype == TRLX_BF16)
        return d_kv == 64 ? k_t5_decode_attn<BF16T, 64, kT5Self, true> : k_t5_decode_attn<BF16T, 128, kT5Self, true>;
    return d_kv == 64 ? k_t5_decode_attn<F32T, 64, kT5Self, true> : k_t5_decode_attn<F32T, 128, kT5Self, true>;
}

extern "C" int trlx_t5_decode_attn_dev(const TrlxT5DecodeAttnArgs* a, const int64_t* clock, void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 decode attention: NULL arguments");
    TRLX_REQUIRE(a->mode == TRLX_T5_ATTN_SELF, TRLX_ERR_ARG,
                 "t5 decode attention, device clock: mode %d (the self-attention only; the cross step reads no t)",
                 a->mode);
    TRLX_REQUIRE(clock, TRLX_ERR_ARG, "t5 decode attention, device clock: NULL clock");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(clock) & 7u) == 0, TRLX_ERR_ARG,
                 "t5 decode attention, device clock: the clock is not aligned to 8 bytes");
    T5AttnDevArgs k;
    const int rc = t5_decode_attn_prepare(a, true, &k.a);
    if (rc) return rc;
    k.clock = clock;
    hipLaunchKernelGGL(t5_pick_clock(a->dtype, a->d_kv), dim3(unsigned(a->B * a->n_heads)), dim3(kT5Threads), 0,
                       (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn<clock>");
}

typedef void (*t5_live_kernel_t)(const T5AttnLiveArgs);
template <class DT, int DKV>
static t5_live_kernel_t t5_pick_live_mode(int mode, bool clock) {
    if (mode == kT5Self)
        return clock ? k_t5_decode_attn<DT, DKV, kT5Self, true, true> : k_t5_decode_attn<DT, DKV, kT5Self, false, true>;
    return mode == kT5Cross ? k_t5_decode_attn<DT, DKV, kT5Cross, false, true>
                            : k_t5_decode_attn<DT, DKV, kT5CrossMasked, false, true>;
}
static t5_live_kernel_t t5_pick_live(int dtype, int64_t d_kv, int mode, bool clock) {
    if (dtype == TRLX_BF16)
        return d_kv == 64 ? t5_pick_live_mode<BF16T, 64>(mode, clock) : t5_pick_live_mode<BF16T, 128>(mode, clock);
    return d_kv == 64 ? t5_pick_live_mode<F32T, 64>(mode, clock) : t5_pick_live_mode<F32T, 128>(mode, clock);
}

extern "C" int trlx_t5_decode_attn_live(const TrlxT5DecodeAttnArgs* a, const int64_t* live, const int64_t* clock,
                                        void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 decode attention: NULL arguments");
    TRLX_REQUIRE(live, TRLX_ERR_ARG, "t5 decode attention, live rows: NULL live");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(live) & 7u) == 0, TRLX_ERR_ARG,
                 "t5 decode attention, live rows: live is not aligned to 8 bytes");
    TRLX_REQUIRE(!clock || a->mode == TRLX_T5_ATTN_SELF, TRLX_ERR_ARG,
                 "t5 decode attention, live rows: a clock with mode %d (the self-attention only; the cross step "
                 "reads no t)", a->mode);
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(clock) & 7u) == 0, TRLX_ERR_ARG,
                 "t5 decode attention, live rows: the clock is not aligned to 8 bytes");
    T5AttnLiveArgs k;
    const int rc = t5_decode_attn_prepare(a, clock != nullptr, &k.a);
    if (rc) return rc;
    k.clock = clock;
    k.live = live;
    const int mode = a->mode == TRLX_T5_ATTN_SELF ? kT5Self : a->key_mask ? kT5CrossMasked : kT5Cross;
    hipLaunchKernelGGL(t5_pick_live(a->dtype, a->d_kv, mode, clock != nullptr), dim3(unsigned(a->B * a->n_heads)),
                       dim3(kT5Threads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn<live>");
}
