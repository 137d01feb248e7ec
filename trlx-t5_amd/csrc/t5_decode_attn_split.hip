// The decode cross-attention with the encoder keys of a (row, head) split across workgroups: two
// launches in stream order, no atomics, no counters, no spinning.  See trlx_t5_decode_attn_split in
// trlx_t5_amd.h.  The interface is the grouped entry's (t5_decode_attn_group.hip): P prompts, G
// samples a prompt, row b = p * G + g, K / V through element strides, key_mask per prompt, live per
// row.  G = 1 is the plain cross-attention.
//
// k_t5_decode_attn_split_part, grid (P * nH, tiles, X): workgroup (ph, tile, x) is
// k_t5_decode_attn_group restricted to the keys [x * C, min(S, (x + 1) * C)): the same 256 threads,
// LPR, KPW and NG, group gg walks x * C + gg, x * C + gg + NG, ... two in flight, t5_group_step per
// (key, query), the same `on` word, the same LDS merge in group order.  C is a multiple of NG, so
// key j is walked by group j % NG as in the unsplit kernel.  The workgroup stops before the
// division: per live query it writes the unnormalised state (M, L, o[d_kv]) in fp32 to the
// workspace, M = -inf and L = 0 when the range held no live key.  A tile whose queries are all dead
// writes nothing and forms no address into q, K, V or the mask; a dead query of a live tile writes
// nothing either.
//
// k_t5_decode_attn_split_merge: one thread per two outputs of a (row, head) reads the row's states
// in split order, M = max M_x, and for every x with M_x != -inf  w = expf(M_x - M),
// L = fmaf(L_x, w, L), o = fmaf(o_x, w, o); then o / L (zeros when no key was live) and one rounding.
// A dead row gets zeros and its states are not read.
//
// The result depends on X and on nothing else: not on P, the strides or the query tile.  It is not
// the unsplit kernel's bits for X > 1: the unsplit merge weighs all NG groups against one maximum,
// here the groups of a range are weighed against the range's maximum and the ranges against the
// global one, so the roundings of expf and of the sums fall differently.  With one range holding
// every live key the weights of the merge are expf(0) = 1 and the bits are the unsplit kernel's.
//
// Kernels in a translation unit of their own: t5_decode_attn.hip, t5_cross_kv8.hip,
// t5_decode_attn_group.hip and their code objects are as they were.
#include <type_traits>

#include "common.h"

namespace trlx {

int t5_group_tile_cap();   // t5_decode_attn_group.hip: the cap trlx_t5_decode_attn_group_tile set, or the default

constexpr int kT5SThreads = 256;
constexpr int kT5SWaves = kT5SThreads / kWave;
constexpr int kT5SPark = 4;       // queries whose states are parked in LDS at a time
constexpr int kT5SMaxSplits = 8;  // the largest X the entry takes

struct T5AttnSplitArgs {
    const void* q;
    const void* k;
    const void* v;
    const int64_t* mask;    // [P, S] or NULL (MASKED = false)
    const int64_t* live;    // [P * G] or NULL (LIVE = false)
    float* ws;              // [P * G, nH, X, DKV + 2]: M, L, o[DKV]
    void* out;
    int64_t ldq;
    int64_t k_sp, k_sh, k_ss, v_sp, v_sh, v_ss;   // element strides over (p, h, s)
    int nH, G, S;
    int C, X;               // keys a range, ranges launched
    int rows;               // P * G
};

// t5_group_step of t5_decode_attn_group.hip, operation for operation.
template <int EPV, int LPR>
__device__ __forceinline__ void t5_split_step(const float (&qf)[EPV], const float (&kf)[EPV], const float (&vf)[EPV],
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

// blockIdx.x = p * nH + h, blockIdx.y = the query tile, blockIdx.z = the key range.
template <class DT, int DKV, bool MASKED, bool LIVE, int GT>
__global__ __launch_bounds__(kT5SThreads) void k_t5_decode_attn_split_part(const T5AttnSplitArgs a) {
    typedef typename DT::elem_t E;
    constexpr int EPV = DT::kEPV;
    constexpr int LPR = DKV / EPV;             // lanes per key row
    constexpr int KPW = kWave / LPR;           // key rows per wave-wide load
    constexpr int NG = kT5SWaves * KPW;        // groups per workgroup
    constexpr int QR = GT < kT5SPark ? GT : kT5SPark;
    constexpr int REC = DKV + 2;               // floats of one state
    static_assert(DKV % EPV == 0 && kWave % LPR == 0 && LPR >= 2, "row geometry");
    static_assert(GT >= 1 && GT <= 8 && GT % QR == 0 && QR * (DKV / 2) <= kT5SThreads, "query tile");
    __shared__ float s_acc[QR * NG * DKV];
    __shared__ float s_m[QR * NG];
    __shared__ float s_l[QR * NG];

    const int ph = blockIdx.x;
    const int p = ph / a.nH, h = ph - p * a.nH;
    const int g0 = int(blockIdx.y) * GT;
    const int nq = a.G - g0 < GT ? a.G - g0 : GT;
    const int x = blockIdx.z;
    const int64_t b0 = int64_t(p) * a.G + g0;  // the tile's first row of q / live / the workspace
    unsigned on = (1u << nq) - 1u;
    if constexpr (LIVE) {
#pragma unroll
        for (int i = 0; i < GT; ++i)
            if (i < nq && a.live[b0 + i] == 0) on &= ~(1u << i);
        if (on == 0) return;   // block-uniform: no state; the merge reads none of a dead row
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

    const int lo = x * a.C;                    // a multiple of NG; lo < S by the launch
    const int n = a.S - lo < a.C ? a.S : lo + a.C;
    // ALL: every query of the tile is on, so the GT steps of a key carry no branch between them
    auto walk = [&](auto all) {
        constexpr bool ALL = decltype(all)::value;
        auto apply = [&](const vec4u& kv, const vec4u& vv) {
            float kf[EPV], vf[EPV];
            DT::unpack(kv, kf);
            DT::unpack(vv, vf);
#pragma unroll
            for (int i = 0; i < GT; ++i)
                if (ALL || ((on >> i) & 1u)) t5_split_step<EPV, LPR>(qf[i], kf, vf, m[i], l[i], acc[i]);
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

    // merge, QR queries at a time: every group parks (m, l, its slice of P·V) of each of them, then
    // d_kv / 2 threads per query combine the groups in group order; no division, no rounding
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
        if (i < QR && qi < nq && ((on >> qi) & 1u)) {   // a dead query: no state
            const int d = 2 * (threadIdx.x - i * (DKV / 2));
            const float* sm = s_m + i * NG;
            const float* sL = s_l + i * NG;
            const float* sa = s_acc + i * NG * DKV;
            float o0 = 0.f, o1 = 0.f;
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
            // no live key in the range: M = -inf, L = 0 (and o = 0) as they stand
            float* rec = a.ws + (((b0 + qi) * a.nH + h) * a.X + x) * REC;
            float2 r;
            if (d == 0) {
                r.x = M;
                r.y = L;
                *reinterpret_cast<float2*>(rec) = r;
            }
            r.x = o0;
            r.y = o1;
            *reinterpret_cast<float2*>(rec + 2 + d) = r;
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

// Thread t of the grid: outputs d, d + 1 of (row, head) = t / (DKV / 2).
template <class DT, int DKV, bool LIVE>
__global__ __launch_bounds__(kT5SThreads) void k_t5_decode_attn_split_merge(const T5AttnSplitArgs a) {
    typedef typename DT::elem_t E;
    constexpr int REC = DKV + 2;
    const int64_t t = int64_t(blockIdx.x) * kT5SThreads + threadIdx.x;
    const int64_t bh = t / (DKV / 2);
    if (bh >= int64_t(a.rows) * a.nH) return;
    const int d = 2 * int(t - bh * (DKV / 2));
    float o0 = 0.f, o1 = 0.f;
    bool dead = false;
    if constexpr (LIVE) dead = a.live[bh / a.nH] == 0;
    if (!dead) {
        const float* rec = a.ws + bh * a.X * REC;
        float M = rec[0];
        for (int x = 1; x < a.X; ++x) M = fmaxf(M, rec[x * REC]);
        float L = 0.f;
        for (int x = 0; x < a.X; ++x) {
            const float2 ml = *reinterpret_cast<const float2*>(rec + x * REC);
            if (ml.x == -INFINITY) continue;   // a range that held no live key
            const float2 o = *reinterpret_cast<const float2*>(rec + x * REC + 2 + d);
            const float w = expf(ml.x - M);
            L = fmaf(ml.y, w, L);
            o0 = fmaf(o.x, w, o0);
            o1 = fmaf(o.y, w, o1);
        }
        // no live key at all (a fully masked prompt): zeros
        const bool any = L > 0.f || L != L;
        o0 = any ? o0 / L : 0.f;
        o1 = any ? o1 / L : 0.f;
    }
    const int64_t o = bh * DKV + d;
    if (sizeof(E) == 2) {
        *reinterpret_cast<uint32_t*>(static_cast<uint16_t*>(a.out) + o) = pack_bf2(o0, o1);
    } else {
        float2 r;
        r.x = o0;
        r.y = o1;
        *reinterpret_cast<float2*>(static_cast<float*>(a.out) + o) = r;
    }
}

typedef void (*t5_split_kernel_t)(const T5AttnSplitArgs);
template <class DT, int DKV, int GT>
static t5_split_kernel_t t5_split_pick_flags(bool masked, bool live) {
    if (live)
        return masked ? k_t5_decode_attn_split_part<DT, DKV, true, true, GT>
                      : k_t5_decode_attn_split_part<DT, DKV, false, true, GT>;
    return masked ? k_t5_decode_attn_split_part<DT, DKV, true, false, GT>
                  : k_t5_decode_attn_split_part<DT, DKV, false, false, GT>;
}
template <class DT, int DKV>
static t5_split_kernel_t t5_split_pick_tile(int gt, bool masked, bool live) {
    return gt == 8   ? t5_split_pick_flags<DT, DKV, 8>(masked, live)
           : gt == 4 ? t5_split_pick_flags<DT, DKV, 4>(masked, live)
           : gt == 2 ? t5_split_pick_flags<DT, DKV, 2>(masked, live)
                     : t5_split_pick_flags<DT, DKV, 1>(masked, live);
}
static t5_split_kernel_t t5_split_pick_part(int dtype, int64_t d_kv, int gt, bool masked, bool live) {
    if (dtype == TRLX_BF16)
        return d_kv == 64 ? t5_split_pick_tile<BF16T, 64>(gt, masked, live) : t5_split_pick_tile<BF16T, 128>(gt, masked, live);
    return d_kv == 64 ? t5_split_pick_tile<F32T, 64>(gt, masked, live) : t5_split_pick_tile<F32T, 128>(gt, masked, live);
}
template <class DT, int DKV>
static t5_split_kernel_t t5_split_pick_merge_live(bool live) {
    return live ? k_t5_decode_attn_split_merge<DT, DKV, true> : k_t5_decode_attn_split_merge<DT, DKV, false>;
}
static t5_split_kernel_t t5_split_pick_merge(int dtype, int64_t d_kv, bool live) {
    if (dtype == TRLX_BF16)
        return d_kv == 64 ? t5_split_pick_merge_live<BF16T, 64>(live) : t5_split_pick_merge_live<BF16T, 128>(live);
    return d_kv == 64 ? t5_split_pick_merge_live<F32T, 64>(live) : t5_split_pick_merge_live<F32T, 128>(live);
}

// NG of the kernels' geometry: 4 waves * (64 lanes / (d_kv / elements a 16-byte vector)).
static int t5_split_groups(int dtype, int64_t d_kv) {
    const int epv = dtype == TRLX_BF16 ? 8 : 4;
    return kT5SWaves * (kWave / int(d_kv / epv));
}
// C: ceil(S / X) rounded up to a multiple of NG.
static int64_t t5_split_range(int64_t S, int64_t X, int ng) {
    const int64_t c = (S + X - 1) / X;
    return (c + ng - 1) / ng * ng;
}
static bool t5_split_geometry_ok(int dtype, int64_t d_kv) {
    return (dtype == TRLX_BF16 || dtype == TRLX_F32) && (d_kv == 64 || d_kv == 128);
}
// the tile trlx_t5_decode_attn_group takes for G under the cap
static int t5_split_tile(int64_t G) {
    const int cap = t5_group_tile_cap();
    int gt = 1;
    while (gt < cap && gt < G) gt *= 2;
    return gt;
}

}  // namespace trlx

using namespace trlx;

extern "C" int64_t trlx_t5_decode_attn_split_workspace_bytes(int64_t rows, int64_t n_heads, int64_t d_kv, int64_t splits) {
    if (rows < 1 || n_heads < 1 || (d_kv != 64 && d_kv != 128) || splits < 1 || splits > kT5SMaxSplits) return 0;
    if (rows > 0x7fffffffLL || n_heads > 0x7fffffffLL / 128 || rows * n_heads > 0x7fffffffLL) return 0;
    return rows * n_heads * splits * (d_kv + 2) * int64_t(sizeof(float));
}

extern "C" int trlx_t5_decode_attn_split_geometry(int dtype, int64_t d_kv, int64_t S, int64_t splits,
                                                  TrlxT5DecodeAttnSplitGeometry* g) {
    TRLX_REQUIRE(g, TRLX_ERR_ARG, "t5 split decode attention geometry: NULL result");
    *g = TrlxT5DecodeAttnSplitGeometry{};
    TRLX_REQUIRE(t5_split_geometry_ok(dtype, d_kv), TRLX_ERR_ARG,
                 "t5 split decode attention geometry: dtype %d, d_kv %lld (bf16 / fp32, 64 / 128)", dtype, (long long)d_kv);
    TRLX_REQUIRE(S >= 1 && S <= 0x7fffffffLL / 128, TRLX_ERR_ARG, "t5 split decode attention geometry: S %lld", (long long)S);
    TRLX_REQUIRE(splits >= 1 && splits <= kT5SMaxSplits, TRLX_ERR_ARG,
                 "t5 split decode attention geometry: splits %lld (1 to %d)", (long long)splits, kT5SMaxSplits);
    g->NG = t5_split_groups(dtype, d_kv);
    g->C = t5_split_range(S, splits, int(g->NG));
    g->ranges = (S + g->C - 1) / g->C;
    g->tile = t5_group_tile_cap();
    g->max_splits = kT5SMaxSplits;
    return TRLX_OK;
}

// The X taken for splits == 0.  A pure function of the shape: not of live, not of the device, not
// of the tile knob (W below counts tiles of the default cap).  Set from
// profiles/t5_cross_split_bench.json ("Encoder keys split across workgroups"):
// per shape class the X whose median inside a replayed graph beat the best existing route by more
// than that route's own min-max spread, 1 where none did.  W = the unsplit grid, R = the keys a
// group walks.
//   W > 256               1   measured at W 768 (P 64 x G 4, P 32 x G 8), 3072 (B 256) and 4096: every X loses or ties
//   R < 32                1   measured at R 16 (T5-base S 512, W 96 and W 24): a tie with the plain call, a loss to it
//   W <= 64               8   W 24, R 64 (P 2 x G 4, S 2048): 22.2 us against 33.3 (X 4: 25.1)
//   W <= 128              4   W 96, R 64 (T5-base B 8, S 2048): 18.9 us against 32.4 (X 2: 22.9, X 8: 21.3)
//   W <= 256              2   W 256, R 32 and R 128 (nH 32, d 128, B 8): 18.3 against 21.1, 55.4 against 81.3 (X 4: 20.2, 57.1)
// and X halved until a range keeps 8 keys a group, the shortest range that was measured to win.
// fp32 was not measured: 1.
extern "C" int trlx_t5_decode_attn_split_plan(int dtype, int64_t P, int64_t G, int64_t n_heads, int64_t d_kv, int64_t S) {
    if (!t5_split_geometry_ok(dtype, d_kv) || P < 1 || G < 1 || n_heads < 1 || S < 1) return 1;
    if (dtype != TRLX_BF16) return 1;
    int64_t tile = 1;   // the default cap's tile, whatever the knob says
    while (tile < 4 && tile < G) tile *= 2;
    if (P > 256 || n_heads > 256 || G > 1024) return 1;
    const int64_t W = P * n_heads * ((G + tile - 1) / tile);
    if (W > 256) return 1;
    const int ng = t5_split_groups(dtype, d_kv);
    const int64_t R = (S + ng - 1) / ng;
    if (R < 32) return 1;
    int X = W <= 64 ? 8 : W <= 128 ? 4 : 2;
    while (X > 1 && R / X < 8) X /= 2;
    return X;
}

extern "C" int trlx_t5_decode_attn_split(const TrlxT5DecodeAttnGroupArgs* a, int64_t splits, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 split decode attention: NULL arguments");
    TRLX_REQUIRE(a->dtype == TRLX_BF16 || a->dtype == TRLX_F32, TRLX_ERR_ARG,
                 "t5 split decode attention: dtype %d (bf16 and fp32 only)", a->dtype);
    TRLX_REQUIRE(a->d_kv == 64 || a->d_kv == 128, TRLX_ERR_ARG, "t5 split decode attention: d_kv %lld (64 and 128 only)",
                 (long long)a->d_kv);
    TRLX_REQUIRE(a->P >= 1 && a->G >= 1 && a->n_heads >= 1 && a->S >= 1, TRLX_ERR_ARG,
                 "t5 split decode attention: P %lld, G %lld, heads %lld, S %lld (all >= 1)", (long long)a->P,
                 (long long)a->G, (long long)a->n_heads, (long long)a->S);
    // the grid is (P * heads, ceil(G / tile), X); rows, heads and keys are 32-bit in the kernels
    TRLX_REQUIRE(a->P <= 0x7fffffffLL && a->G <= 0x7fffffffLL && a->n_heads <= 0x7fffffffLL / 128 &&
                     a->S <= 0x7fffffffLL / 128 && a->P * a->n_heads <= 0x7fffffffLL && a->P * a->G <= 0x7fffffffLL &&
                     a->P * a->G * a->n_heads <= 0x7fffffffLL,
                 TRLX_ERR_ARG, "t5 split decode attention: P %lld, G %lld, heads %lld, S %lld overflow the grid",
                 (long long)a->P, (long long)a->G, (long long)a->n_heads, (long long)a->S);
    TRLX_REQUIRE(a->q && a->k && a->v && a->out, TRLX_ERR_ARG, "t5 split decode attention: NULL q / K / V / out");
    const int64_t inner = a->n_heads * a->d_kv;
    const int64_t epv = a->dtype == TRLX_BF16 ? 8 : 4;
    const int64_t ldq = a->P * a->G == 1 ? inner : a->ldq;   // a single row has no stride to speak of
    TRLX_REQUIRE(ldq >= inner && ldq % epv == 0, TRLX_ERR_ARG,
                 "t5 split decode attention: q row stride %lld (>= heads * d_kv = %lld, whole 16-byte vectors)",
                 (long long)ldq, (long long)inner);
    // a dimension of size 1 has no stride to speak of
    const int64_t st[6] = {a->P > 1 ? a->k_stride_p : 0, a->n_heads > 1 ? a->k_stride_h : 0, a->S > 1 ? a->k_stride_s : 0,
                           a->P > 1 ? a->v_stride_p : 0, a->n_heads > 1 ? a->v_stride_h : 0, a->S > 1 ? a->v_stride_s : 0};
    for (int i = 0; i < 6; ++i)
        TRLX_REQUIRE(st[i] >= 0 && st[i] % epv == 0, TRLX_ERR_ARG,
                     "t5 split decode attention: stride %lld (non-negative, whole 16-byte vectors)", (long long)st[i]);
    TRLX_REQUIRE((a->S == 1 || (st[2] >= a->d_kv && st[5] >= a->d_kv)) &&
                     (a->n_heads == 1 || (st[1] >= a->d_kv && st[4] >= a->d_kv)),
                 TRLX_ERR_ARG, "t5 split decode attention: key and head strides must be at least d_kv");
    auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    TRLX_REQUIRE(!mis(a->q, 15) && !mis(a->k, 15) && !mis(a->v, 15) && !mis(a->out, 15), TRLX_ERR_ARG,
                 "t5 split decode attention: q, K, V and out must be 16-byte aligned");
    TRLX_REQUIRE(!mis(a->key_mask, 7) && !mis(a->live, 7), TRLX_ERR_ARG,
                 "t5 split decode attention: key_mask and live must be 8-byte aligned");
    const int gt = t5_split_tile(a->G);
    const int64_t tiles = (a->G + gt - 1) / gt;
    TRLX_REQUIRE(tiles <= 65535, TRLX_ERR_ARG, "t5 split decode attention: G %lld gives %lld query tiles (at most 65535)",
                 (long long)a->G, (long long)tiles);
    TRLX_REQUIRE(splits >= 0 && splits <= kT5SMaxSplits, TRLX_ERR_ARG,
                 "t5 split decode attention: splits %lld (0 = the plan, 1 to %d)", (long long)splits, kT5SMaxSplits);
    const int64_t X = splits ? splits : trlx_t5_decode_attn_split_plan(a->dtype, a->P, a->G, a->n_heads, a->d_kv, a->S);
    const int64_t need = trlx_t5_decode_attn_split_workspace_bytes(a->P * a->G, a->n_heads, a->d_kv, X);
    TRLX_REQUIRE(workspace && !mis(workspace, 15) && workspace_bytes >= need, TRLX_ERR_ARG,
                 "t5 split decode attention: workspace %p of %lld bytes (16-byte aligned, at least %lld bytes for %lld splits)",
                 workspace, (long long)workspace_bytes, (long long)need, (long long)X);
    if (X == 1) return trlx_t5_decode_attn_group(a, stream);   // one range: the unsplit kernel, one launch

    const int ng = t5_split_groups(a->dtype, a->d_kv);
    const int64_t C = t5_split_range(a->S, X, ng);
    const int64_t ranges = (a->S + C - 1) / C;   // the non-empty ones, <= X
    T5AttnSplitArgs k = {};
    k.q = a->q;
    k.k = a->k;
    k.v = a->v;
    k.mask = a->key_mask;
    k.live = a->live;
    k.ws = static_cast<float*>(workspace);
    k.out = a->out;
    k.ldq = ldq;
    k.k_sp = st[0], k.k_sh = st[1], k.k_ss = st[2];
    k.v_sp = st[3], k.v_sh = st[4], k.v_ss = st[5];
    k.nH = int(a->n_heads);
    k.G = int(a->G);
    k.S = int(a->S);
    k.C = int(C);
    k.X = int(ranges);
    k.rows = int(a->P * a->G);
    hipLaunchKernelGGL(t5_split_pick_part(a->dtype, a->d_kv, gt, a->key_mask != nullptr, a->live != nullptr),
                       dim3(unsigned(a->P * a->n_heads), unsigned(tiles), unsigned(ranges)), dim3(kT5SThreads), 0,
                       (hipStream_t)stream, k);
    const int rc = check_launch("k_t5_decode_attn_split_part");
    if (rc != TRLX_OK) return rc;
    const int64_t threads = a->P * a->G * a->n_heads * (a->d_kv / 2);
    hipLaunchKernelGGL(t5_split_pick_merge(a->dtype, a->d_kv, a->live != nullptr),
                       dim3(unsigned((threads + kT5SThreads - 1) / kT5SThreads)), dim3(kT5SThreads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn_split_merge");
}
