// The decode cross-attention over encoder keys / values that the G samples of a prompt share: one
// launch, one workgroup per (prompt, head, tile of up to GT queries).  See trlx_t5_decode_attn_group
// in trlx_t5_amd.h.  Row b = p * G + g of q / out / live is sample g of prompt p, the order of
// repeat_interleave(G, dim = 0).
//
// The geometry is k_t5_decode_attn's (t5_decode_attn.hip), unchanged: 256 threads, LPR = d_kv / EPV
// lanes a key row, KPW = 64 / LPR rows a wave-wide load, NG = 4 * KPW groups, group gg walks keys
// gg, gg + NG, ... two in flight, the groups' states merged through LDS in group order by d_kv / 2
// threads, one rounding.  What differs: a group holds GT query slices and GT online-softmax states,
// and every (k, v) pair it loads is applied to all of them by t5_group_step, whose arithmetic is the
// step of k_t5_decode_attn operation for operation.  Per query the sequence of floating-point
// operations is therefore that kernel's, and so are the bits: K / V bytes per token drop by G and
// nothing else changes.  The states are parked in LDS four queries at a time (32 KB at most) and
// each query is merged by its own d_kv / 2 threads.
//
// Kernels and an argument block of their own in a translation unit of their own: t5_decode_attn.hip,
// t5_cross_kv8.hip and their code objects are as they were.
#include <type_traits>

#include "common.h"

namespace trlx {

constexpr int kT5GThreads = 256;
constexpr int kT5GWaves = kT5GThreads / kWave;
constexpr int kT5GPark = 4;   // queries whose states are parked in LDS at a time

struct T5AttnGroupArgs {
    const void* q;
    const void* k;
    const void* v;
    const int64_t* mask;    // [P, S] or NULL (MASKED = false)
    const int64_t* live;    // [P * G] or NULL (LIVE = false)
    void* out;
    int64_t ldq;
    int64_t k_sp, k_sh, k_ss, v_sp, v_sh, v_ss;   // element strides over (p, h, s)
    int nH, G, S;
};

// One key applied to one query: the step of k_t5_decode_attn with no bias (the cross mode), written
// once and called per query.  kf / vf are the key / value row slices unpacked to fp32 (exact).
template <int EPV, int LPR>
__device__ __forceinline__ void t5_group_step(const float (&qf)[EPV], const float (&kf)[EPV], const float (&vf)[EPV],
                                              float& m, float& l, float (&acc)[EPV]) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EPV; ++e) s = fmaf(qf[e], kf[e], s);
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
    s += 0.f;   // the bias add of the cross mode
    const float mn = fmaxf(m, s);
    const float sc = expf(m - mn), p = expf(s - mn);
    l = fmaf(l, sc, p);
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = fmaf(acc[e], sc, p * vf[e]);
    m = mn;
}

template <class E, int DKV>
__device__ __forceinline__ void t5_group_store(void* out, int64_t o, float o0, float o1) {
    if (sizeof(E) == 2) {
        *reinterpret_cast<uint32_t*>(static_cast<uint16_t*>(out) + o) = pack_bf2(o0, o1);
    } else {
        float2 r;
        r.x = o0;
        r.y = o1;
        *reinterpret_cast<float2*>(static_cast<float*>(out) + o) = r;
    }
}

// blockIdx.x = p * nH + h, blockIdx.y = the tile: queries g0 = tile * GT ... g0 + nq - 1 of prompt p.
// `on` holds one bit per query of the tile: set for a query that exists (a remainder tile has nq <
// GT) and, with LIVE, whose live word is non-zero.  Every decision taken from it is
// workgroup-uniform.  on == 0: zeros to the tile's out rows and out, before any barrier and before
// any address into q, K, V or the mask is formed.
template <class DT, int DKV, bool MASKED, bool LIVE, int GT>
__global__ __launch_bounds__(kT5GThreads) void k_t5_decode_attn_group(const T5AttnGroupArgs a) {
    typedef typename DT::elem_t E;
    constexpr int EPV = DT::kEPV;
    constexpr int LPR = DKV / EPV;             // lanes per key row
    constexpr int KPW = kWave / LPR;           // key rows per wave-wide load
    constexpr int NG = kT5GWaves * KPW;        // groups per workgroup
    constexpr int QR = GT < kT5GPark ? GT : kT5GPark;
    static_assert(DKV % EPV == 0 && kWave % LPR == 0 && LPR >= 2, "row geometry");
    static_assert(GT >= 1 && GT <= 8 && GT % QR == 0 && QR * (DKV / 2) <= kT5GThreads, "query tile");
    __shared__ float s_acc[QR * NG * DKV];
    __shared__ float s_m[QR * NG];
    __shared__ float s_l[QR * NG];

    const int ph = blockIdx.x;
    const int p = ph / a.nH, h = ph - p * a.nH;
    const int g0 = int(blockIdx.y) * GT;
    const int nq = a.G - g0 < GT ? a.G - g0 : GT;
    const int64_t b0 = int64_t(p) * a.G + g0;  // the tile's first row of q / out / live
    unsigned on = (1u << nq) - 1u;
    if constexpr (LIVE) {
#pragma unroll
        for (int i = 0; i < GT; ++i)
            if (i < nq && a.live[b0 + i] == 0) on &= ~(1u << i);
        if (on == 0) {   // block-uniform
            if (threadIdx.x < DKV / 2)
                for (int i = 0; i < nq; ++i)
                    t5_group_store<E, DKV>(a.out, ((b0 + i) * a.nH + h) * DKV + 2 * threadIdx.x, 0.f, 0.f);
            return;
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int sl = lane % LPR;                 // this lane's vector of the row
    const int gg = wave * KPW + lane / LPR;    // group id in the workgroup
    const int col = h * DKV + sl * EPV;

    float qf[GT][EPV], m[GT], l[GT], acc[GT][EPV];
#pragma unroll
    for (int i = 0; i < GT; ++i) {
        m[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
            acc[i][e] = 0.f;
            qf[i][e] = 0.f;
        }
        if ((on >> i) & 1u)   // a dead query's q row is not read
            DT::unpack(*reinterpret_cast<const vec4u*>(static_cast<const E*>(a.q) + (b0 + i) * a.ldq + col), qf[i]);
    }
    const E* K = static_cast<const E*>(a.k) + int64_t(p) * a.k_sp + int64_t(h) * a.k_sh + sl * EPV;
    const E* V = static_cast<const E*>(a.v) + int64_t(p) * a.v_sp + int64_t(h) * a.v_sh + sl * EPV;
    const int64_t* mask = MASKED ? a.mask + int64_t(p) * a.S : nullptr;

    const int n = a.S;
    // ALL: every query of the tile is on, so the GT steps of a key carry no branch between them
    auto walk = [&](auto all) {
        constexpr bool ALL = decltype(all)::value;
        auto apply = [&](const vec4u& kv, const vec4u& vv) {
            float kf[EPV], vf[EPV];
            DT::unpack(kv, kf);
            DT::unpack(vv, vf);
#pragma unroll
            for (int i = 0; i < GT; ++i)
                if (ALL || ((on >> i) & 1u)) t5_group_step<EPV, LPR>(qf[i], kf, vf, m[i], l[i], acc[i]);
        };
#pragma unroll 1
        for (int j0 = gg; j0 < n; j0 += 2 * NG) {
            const int j1 = j0 + NG;
            bool live0 = true, live1 = j1 < n;
            if (MASKED) {
                live0 = mask[j0] != 0;
                live1 = live1 && mask[j1] != 0;
            }
            vec4u k0 = vec4u_make(0, 0, 0, 0), v0 = k0, k1 = k0, v1 = k0;
            if (live0) {
                k0 = *reinterpret_cast<const vec4u*>(K + int64_t(j0) * a.k_ss);
                v0 = *reinterpret_cast<const vec4u*>(V + int64_t(j0) * a.v_ss);
            }
            if (live1) {
                k1 = *reinterpret_cast<const vec4u*>(K + int64_t(j1) * a.k_ss);
                v1 = *reinterpret_cast<const vec4u*>(V + int64_t(j1) * a.v_ss);
            }
            if (live0) apply(k0, v0);
            if (live1) apply(k1, v1);
        }
    };
    if (on == (1u << GT) - 1u)   // block-uniform
        walk(std::true_type{});
    else
        walk(std::false_type{});

    // merge, QR queries at a time: every group parks (m, l, its slice of P·V) of each of them, then
    // d_kv / 2 threads per query combine the groups in group order, divide and round once
    auto merge = [&](auto first) {
        constexpr int r0 = decltype(first)::value;
#pragma unroll
        for (int i = 0; i < QR; ++i) {
#pragma unroll
            for (int e = 0; e < EPV; ++e) s_acc[(i * NG + gg) * DKV + sl * EPV + e] = acc[r0 + i][e];
            if (sl == 0) {
                s_m[i * NG + gg] = m[r0 + i];
                s_l[i * NG + gg] = l[r0 + i];
            }
        }
        __syncthreads();
        const int i = threadIdx.x / (DKV / 2), qi = r0 + i;
        if (i < QR && qi < nq) {
            const int d = 2 * (threadIdx.x - i * (DKV / 2));
            const float* sm = s_m + i * NG;
            const float* sL = s_l + i * NG;
            const float* sa = s_acc + i * NG * DKV;
            float o0 = 0.f, o1 = 0.f;
            if ((on >> qi) & 1u) {
                float M = sm[0];
                for (int g = 1; g < NG; ++g) M = fmaxf(M, sm[g]);
                float L = 0.f;
                for (int g = 0; g < NG; ++g) {
                    const float mg = sm[g];
                    if (mg == -INFINITY) continue;   // a group that saw no live key
                    const float w = expf(mg - M);
                    L = fmaf(sL[g], w, L);
                    o0 = fmaf(sa[g * DKV + d], w, o0);
                    o1 = fmaf(sa[g * DKV + d + 1], w, o1);
                }
                // no live key at all (a fully masked prompt): zeros
                const bool any = L > 0.f || L != L;
                o0 = any ? o0 / L : 0.f;
                o1 = any ? o1 / L : 0.f;
            }
            t5_group_store<E, DKV>(a.out, ((b0 + qi) * a.nH + h) * DKV + d, o0, o1);   // a dead query: zeros
        }
    };
    merge(std::integral_constant<int, 0>{});
    if constexpr (GT > QR) {
        static_assert(GT == 2 * QR, "two rounds at most");
        if (QR < nq) {   // block-uniform
            __syncthreads();   // the first round's reads
            merge(std::integral_constant<int, QR>{});
        }
    }
}

typedef void (*t5_group_kernel_t)(const T5AttnGroupArgs);
template <class DT, int DKV, int GT>
static t5_group_kernel_t t5_group_pick_flags(bool masked, bool live) {
    if (live)
        return masked ? k_t5_decode_attn_group<DT, DKV, true, true, GT> : k_t5_decode_attn_group<DT, DKV, false, true, GT>;
    return masked ? k_t5_decode_attn_group<DT, DKV, true, false, GT> : k_t5_decode_attn_group<DT, DKV, false, false, GT>;
}
template <class DT, int DKV>
static t5_group_kernel_t t5_group_pick_tile(int gt, bool masked, bool live) {
    return gt == 8   ? t5_group_pick_flags<DT, DKV, 8>(masked, live)
           : gt == 4 ? t5_group_pick_flags<DT, DKV, 4>(masked, live)
           : gt == 2 ? t5_group_pick_flags<DT, DKV, 2>(masked, live)
                     : t5_group_pick_flags<DT, DKV, 1>(masked, live);
}
static t5_group_kernel_t t5_group_pick(int dtype, int64_t d_kv, int gt, bool masked, bool live) {
    if (dtype == TRLX_BF16)
        return d_kv == 64 ? t5_group_pick_tile<BF16T, 64>(gt, masked, live) : t5_group_pick_tile<BF16T, 128>(gt, masked, live);
    return d_kv == 64 ? t5_group_pick_tile<F32T, 64>(gt, masked, live) : t5_group_pick_tile<F32T, 128>(gt, masked, live);
}

// The built query tiles are 1, 2, 4 and 8.  kT5GDefaultTile is the largest the entry takes unless
// trlx_t5_decode_attn_group_tile says otherwise.  A G below it takes the smallest built tile that
// holds G, so at T5-base, P 64 x G 4, S 512 a cap of 4 and a cap of 8 launch the same GT 4 kernel
// (33.5 and 32.7 us, the spreads one inside the other); at G 8, where they differ, two GT 4 tiles
// take 32.2 us and one GT 8 tile 44.1 us (profiles/t5_cross_group_bench.json).
constexpr int kT5GDefaultTile = 4;
static TuneKnob g_group_tile = {0};   // 0: kT5GDefaultTile

// host only: the cap in force, for trlx_t5_decode_attn_split (t5_decode_attn_split.hip), which tiles as this entry does
int t5_group_tile_cap() { return g_group_tile ? int(g_group_tile) : kT5GDefaultTile; }

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_decode_attn_group_tile(int64_t tile) {
    TRLX_REQUIRE(tile == 0 || tile == 1 || tile == 2 || tile == 4 || tile == 8, TRLX_ERR_ARG,
                 "t5 grouped decode attention: query tile %lld (0 = default, 1, 2, 4 or 8)", (long long)tile);
    g_group_tile = int(tile);
    return TRLX_OK;
}

extern "C" int trlx_t5_decode_attn_group(const TrlxT5DecodeAttnGroupArgs* a, void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 grouped decode attention: NULL arguments");
    TRLX_REQUIRE(a->dtype == TRLX_BF16 || a->dtype == TRLX_F32, TRLX_ERR_ARG,
                 "t5 grouped decode attention: dtype %d (bf16 and fp32 only)", a->dtype);
    TRLX_REQUIRE(a->d_kv == 64 || a->d_kv == 128, TRLX_ERR_ARG, "t5 grouped decode attention: d_kv %lld (64 and 128 only)",
                 (long long)a->d_kv);
    TRLX_REQUIRE(a->P >= 1 && a->G >= 1 && a->n_heads >= 1 && a->S >= 1, TRLX_ERR_ARG,
                 "t5 grouped decode attention: P %lld, G %lld, heads %lld, S %lld (all >= 1)", (long long)a->P,
                 (long long)a->G, (long long)a->n_heads, (long long)a->S);
    // the grid is (P * heads, ceil(G / tile)); rows, heads and keys are 32-bit in the kernel
    TRLX_REQUIRE(a->P <= 0x7fffffffLL && a->G <= 0x7fffffffLL && a->n_heads <= 0x7fffffffLL / 128 &&
                     a->S <= 0x7fffffffLL / 128 && a->P * a->n_heads <= 0x7fffffffLL && a->P * a->G <= 0x7fffffffLL,
                 TRLX_ERR_ARG, "t5 grouped decode attention: P %lld, G %lld, heads %lld, S %lld overflow the grid",
                 (long long)a->P, (long long)a->G, (long long)a->n_heads, (long long)a->S);
    TRLX_REQUIRE(a->q && a->k && a->v && a->out, TRLX_ERR_ARG, "t5 grouped decode attention: NULL q / K / V / out");
    const int64_t inner = a->n_heads * a->d_kv;
    const int64_t epv = a->dtype == TRLX_BF16 ? 8 : 4;
    const int64_t ldq = a->P * a->G == 1 ? inner : a->ldq;   // a single row has no stride to speak of
    TRLX_REQUIRE(ldq >= inner && ldq % epv == 0, TRLX_ERR_ARG,
                 "t5 grouped decode attention: q row stride %lld (>= heads * d_kv = %lld, whole 16-byte vectors)",
                 (long long)ldq, (long long)inner);
    // a dimension of size 1 has no stride to speak of
    const int64_t st[6] = {a->P > 1 ? a->k_stride_p : 0, a->n_heads > 1 ? a->k_stride_h : 0, a->S > 1 ? a->k_stride_s : 0,
                           a->P > 1 ? a->v_stride_p : 0, a->n_heads > 1 ? a->v_stride_h : 0, a->S > 1 ? a->v_stride_s : 0};
    for (int i = 0; i < 6; ++i)
        TRLX_REQUIRE(st[i] >= 0 && st[i] % epv == 0, TRLX_ERR_ARG,
                     "t5 grouped decode attention: stride %lld (non-negative, whole 16-byte vectors)", (long long)st[i]);
    TRLX_REQUIRE((a->S == 1 || (st[2] >= a->d_kv && st[5] >= a->d_kv)) &&
                     (a->n_heads == 1 || (st[1] >= a->d_kv && st[4] >= a->d_kv)),
                 TRLX_ERR_ARG, "t5 grouped decode attention: key and head strides must be at least d_kv");
    auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    TRLX_REQUIRE(!mis(a->q, 15) && !mis(a->k, 15) && !mis(a->v, 15) && !mis(a->out, 15), TRLX_ERR_ARG,
                 "t5 grouped decode attention: q, K, V and out must be 16-byte aligned");
    TRLX_REQUIRE(!mis(a->key_mask, 7) && !mis(a->live, 7), TRLX_ERR_ARG,
                 "t5 grouped decode attention: key_mask and live must be 8-byte aligned");
    const int cap = g_group_tile ? int(g_group_tile) : kT5GDefaultTile;
    int gt = 1;
    while (gt < cap && gt < a->G) gt *= 2;
    const int64_t tiles = (a->G + gt - 1) / gt;
    TRLX_REQUIRE(tiles <= 65535, TRLX_ERR_ARG, "t5 grouped decode attention: G %lld gives %lld query tiles (at most 65535)",
                 (long long)a->G, (long long)tiles);
    T5AttnGroupArgs k = {};
    k.q = a->q;
    k.k = a->k;
    k.v = a->v;
    k.mask = a->key_mask;
    k.live = a->live;
    k.out = a->out;
    k.ldq = ldq;
    k.k_sp = st[0], k.k_sh = st[1], k.k_ss = st[2];
    k.v_sp = st[3], k.v_sh = st[4], k.v_ss = st[5];
    k.nH = int(a->n_heads);
    k.G = int(a->G);
    k.S = int(a->S);
    hipLaunchKernelGGL(t5_group_pick(a->dtype, a->d_kv, gt, a->key_mask != nullptr, a->live != nullptr),
                       dim3(unsigned(a->P * a->n_heads), unsigned(tiles)), dim3(kT5GThreads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn_group");
}
