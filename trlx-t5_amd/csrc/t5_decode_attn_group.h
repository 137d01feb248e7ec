// The body of the grouped decode cross-attention kernels: k_t5_decode_attn_group
// (t5_decode_attn_group.hip) runs it over all S keys and stores the output, and
// k_t5_decode_attn_split_part (t5_decode_attn_split.hip) runs it over one range of the keys and
// stores the undivided state.  Each kernel stays in its own unit, as a wrapper around this body.
//
// The geometry is k_t5_decode_attn's (t5_decode_row.h): 256 threads, LPR = d_kv / EPV lanes a key
// row, KPW = 64 / LPR rows a wave-wide load, NG = 4 * KPW groups, group gg walks keys gg, gg + NG,
// ... two in flight, the groups' states merged through LDS in group order by d_kv / 2 threads.
// What differs: a group holds GT query slices and GT online-softmax states, and every (k, v) pair
// it loads is applied to all of them by t5_row_step, the step of k_t5_decode_attn.  Per query the
// sequence of floating-point operations is therefore that kernel's, and so are the bits: K / V
// bytes per token drop by G and nothing else changes.  The states are parked in LDS four queries at
// a time (32 KB at most) and each query is merged by its own d_kv / 2 threads.
#pragma once

#include <type_traits>

#include "t5_decode_group_check.h"
#include "t5_decode_row.h"

namespace trlx {

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

// the checked arguments into a kernel's argument block: T5AttnGroupArgs, or one with its fields
template <class Args>
static void t5_group_fill(Args& k, const TrlxT5DecodeAttnGroupArgs* a, const T5GroupChecked& c) {
    k.q = a->q;
    k.k = a->k;
    k.v = a->v;
    k.mask = a->key_mask;
    k.live = a->live;
    k.out = a->out;
    k.ldq = c.ldq;
    k.k_sp = c.st[0], k.k_sh = c.st[1], k.k_ss = c.st[2];
    k.v_sp = c.st[3], k.v_sh = c.st[4], k.v_ss = c.st[5];
    k.nH = int(a->n_heads);
    k.G = int(a->G);
    k.S = int(a->S);
}

// blockIdx.x = p * nH + h, blockIdx.y = the tile: queries g0 = tile * GT ... g0 + nq - 1 of prompt p.
// `on` holds one bit per query of the tile: set for a query that exists (a remainder tile has nq <
// GT) and, with LIVE, whose live word is non-zero.  Every decision taken from it is
// workgroup-uniform.  on == 0: the workgroup leaves before any barrier and before any address into
// q, K, V or the mask is formed.
//
// SPLIT = false: the keys are [0, S); a tile with on == 0 gets zeros in its out rows, and so does a
// dead query of a live tile; a live query's state is divided, rounded once and stored to out.
// SPLIT = true (Args has ws, C and X besides): blockIdx.z = x, the keys are [x * C, min(S, (x + 1)
// * C)) with C a multiple of NG, so key j is walked by group j % NG either way; a dead tile and a
// dead query write nothing; a live query's state (M, L, o[d_kv]) goes to the workspace undivided,
// M = -inf and L = 0 when the range held no live key.
template <class DT, int DKV, bool MASKED, bool LIVE, int GT, bool SPLIT, class Args>
__device__ __forceinline__ void t5_group_body(const Args& a) {
    typedef typename DT::elem_t E;
    constexpr int EPV = DT::kEPV;
    typedef T5RowGeom<EPV, DKV> Geom;
    constexpr int LPR = Geom::LPR, KPW = Geom::KPW, NG = Geom::NG;
    constexpr int QR = GT < kT5GPark ? GT : kT5GPark;
    static_assert(GT >= 1 && GT <= 8 && GT % QR == 0 && QR * (DKV / 2) <= kT5RowThreads, "query tile");
    __shared__ float s_acc[QR * NG * DKV];
    __shared__ float s_m[QR * NG];
    __shared__ float s_l[QR * NG];

    const int ph = blockIdx.x;
    const int p = ph / a.nH, h = ph - p * a.nH;
    const int g0 = int(blockIdx.y) * GT;
    const int nq = a.G - g0 < GT ? a.G - g0 : GT;
    const int64_t b0 = int64_t(p) * a.G + g0;  // the tile's first row of q / out / live / the workspace
    unsigned on = (1u << nq) - 1u;
    if constexpr (LIVE) {
#pragma unroll
        for (int i = 0; i < GT; ++i)
            if (i < nq && a.live[b0 + i] == 0) on &= ~(1u << i);
        if (on == 0) {   // block-uniform
            if constexpr (!SPLIT)
                if (threadIdx.x < DKV / 2)
                    for (int i = 0; i < nq; ++i)
                        t5_store_pair<E>(a.out, ((b0 + i) * a.nH + h) * DKV + 2 * threadIdx.x, 0.f, 0.f);
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

    int lo = 0, n = a.S;                       // the keys walked: [lo, n)
    if constexpr (SPLIT) {
        lo = int(blockIdx.z) * a.C;            // a multiple of NG; lo < S by the launch
        n = a.S - lo < a.C ? a.S : lo + a.C;
    }
    // ALL: every query of the tile is on, so the GT steps of a key carry no branch between them
    auto walk = [&](auto all) {
        constexpr bool ALL = decltype(all)::value;
        auto apply = [&](const vec4u& kv, const vec4u& vv) {
            float kf[EPV], vf[EPV];
            DT::unpack(kv, kf);
            DT::unpack(vv, vf);
#pragma unroll
            for (int i = 0; i < GT; ++i)
                if (ALL || ((on >> i) & 1u)) t5_row_step<LPR>(qf[i], kf, vf, m[i], l[i], acc[i], T5ScoreAdd{0.f});
        };
#pragma unroll 1
        for (int j0 = lo + gg; j0 < n; j0 += 2 * NG) {
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

    // merge, QR queries at a time: every group parks the state of each of them, then d_kv / 2
    // threads per query combine the groups in group order
    auto merge = [&](auto first) {
        constexpr int r0 = decltype(first)::value;
#pragma unroll
        for (int i = 0; i < QR; ++i)
            t5_row_park<DKV>(s_m + i * NG, s_l + i * NG, s_acc + i * NG * DKV, gg, sl, m[r0 + i], l[r0 + i], acc[r0 + i]);
        __syncthreads();
        const int i = threadIdx.x / (DKV / 2), qi = r0 + i;
        if (i >= QR || qi >= nq) return;
        const bool alive = (on >> qi) & 1u;
        if (SPLIT && !alive) return;           // a dead query: no state
        const int d = 2 * (threadIdx.x - i * (DKV / 2));
        T5RowState r = {-INFINITY, 0.f, 0.f, 0.f};
        if (alive) r = t5_row_merge<NG, DKV>(s_m + i * NG, s_l + i * NG, s_acc + i * NG * DKV, d);
        if constexpr (SPLIT) {
            float* rec = a.ws + (((b0 + qi) * a.nH + h) * a.X + int(blockIdx.z)) * (DKV + 2);
            if (d == 0) t5_store_pair<float>(rec, 0, r.M, r.L);
            t5_store_pair<float>(rec, 2 + d, r.o0, r.o1);
        } else {
            if (alive) t5_row_divide(r.L, r.o0, r.o1);
            t5_store_pair<E>(a.out, ((b0 + qi) * a.nH + h) * DKV + d, r.o0, r.o1);   // a dead query: zeros
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

// The kernel of K (a k_t5_decode_attn_group or a k_t5_decode_attn_split_part) for a dtype, a d_kv of
// 64 or 128, a tile of 1, 2, 4 or 8 and the two flags: K::get<DT, DKV, MASKED, LIVE, GT>().
template <class K, class DT, int DKV, int GT>
static auto t5_group_pick_flags(bool masked, bool live) {
    if (live) return masked ? K::template get<DT, DKV, true, true, GT>() : K::template get<DT, DKV, false, true, GT>();
    return masked ? K::template get<DT, DKV, true, false, GT>() : K::template get<DT, DKV, false, false, GT>();
}
template <class K, class DT, int DKV>
static auto t5_group_pick_tile(int gt, bool masked, bool live) {
    return gt == 8   ? t5_group_pick_flags<K, DT, DKV, 8>(masked, live)
           : gt == 4 ? t5_group_pick_flags<K, DT, DKV, 4>(masked, live)
           : gt == 2 ? t5_group_pick_flags<K, DT, DKV, 2>(masked, live)
                     : t5_group_pick_flags<K, DT, DKV, 1>(masked, live);
}
template <class K>
static auto t5_group_pick(int dtype, int64_t d_kv, int gt, bool masked, bool live) {
    if (dtype == TRLX_BF16)
        return d_kv == 64 ? t5_group_pick_tile<K, BF16T, 64>(gt, masked, live) : t5_group_pick_tile<K, BF16T, 128>(gt, masked, live);
    return d_kv == 64 ? t5_group_pick_tile<K, F32T, 64>(gt, masked, live) : t5_group_pick_tile<K, F32T, 128>(gt, masked, live);
}

}  // namespace trlx
