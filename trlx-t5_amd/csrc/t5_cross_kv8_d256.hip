// The decode cross-attention over fp8 encoder keys and values at d_kv 256, the UL2 head size, with
// the keys optionally cut across workgroups.  See trlx_t5_decode_attn_kv8_d256 in trlx_t5_amd.h; the
// bytes and the scales are trlx_t5_cross_kv_quantize's (t5_cross_kv8.hip), whose own attention kernel
// stops at d_kv 128 and is not touched.
//
// Geometry.  A key row is 256 bytes: 16 lanes x one 16-byte vector of 16 e4m3fn elements, so a lane
// group is exactly one DPP row of the wave.  A wave-wide load covers 4 rows, the 4-wave workgroup is
// 16 lane groups, and each group keeps kFlight = 4 keys in flight (4 x 2 x 16 B a lane): one trip of
// the loop is 64 keys.  Group g takes keys j0 + g + 16 f, f = 0 ... 3, of a trip.
//
// The block step.  The 4 keys a group has in flight are one block:
//   - K is unpacked one key at a time (v_cvt_pk_f32_fp8) into an fp32 partial dot of 16 products;
//   - the 4 partial dots are reduced over the DPP row by row_ror 8 / 4 / 2 / 1 adds: VALU, no LDS
//     permute, and every lane of the group ends with the same bits (after the rotation by r the values
//     have period r, so v[l - r/2] == v[l + r/2]);
//   - times k_scale; ONE running-max update and ONE rescale of the accumulator for the block: 5 expf
//     for 4 keys where the per-key step takes 8;
//   - V is unpacked only then, one key at a time, into acc = fmaf(p_f, v_f, acc).
// A masked key of a block has p = 0 by a select and its K / V are not loaded; a block with no live
// key is skipped.  All arithmetic is fp32; v_scale multiplies once at the merge.
//
// The merge inside the workgroup is the 64 / 128 kernel's: the 16 groups park (m, l, acc) in LDS and
// thread t < 128 combines outputs 2t, 2t + 1 in group order against the common maximum.  A group with
// l == 0 saw no live key and is skipped (one live key makes l >= 1, a NaN scale makes it NaN).
//
// The key split.  Grid (B * nH, ranges): workgroup (bh, x) walks the whole trips
// [x * T, min(ntrip, (x + 1) * T)), T = ceil(ntrip / splits).  With one range the workgroup finishes
// (times v_scale, / L, one rounding) and stores.  With more, it writes the unnormalised fp32 state
// (M, L, o[256]) to ws[x][bh][258] and k_t5_decode_attn_kv8_d256_merge, one thread per two outputs,
// combines the ranges in split order the same way.  No atomics, no counters.  A dead row
// (live[b] == 0) forms no address but live's: at one range the workgroup stores zeros, at more the
// part kernel returns and the merge stores them.
#include "t5_decode_row.h"

namespace trlx {

constexpr int kKv8dDkv = 256;
constexpr int kKv8dEpv = 16;                                // elements (bytes) a lane
constexpr int kKv8dFlight = 4;                              // keys a group has in flight: one block
constexpr int kKv8dMaxSplits = 16;
constexpr int kKv8dRec = kKv8dDkv + 2;                      // M, L, o[256]
typedef T5RowGeom<kKv8dEpv, kKv8dDkv> Kv8dGeom;             // LPR 16, KPW 4, NG 16
constexpr int kKv8dTrip = kKv8dFlight * Kv8dGeom::NG;       // 64 keys a workgroup loads per loop turn
static_assert(Kv8dGeom::LPR == 16, "a lane group is one DPP row");

struct T5AttnKv8D256Args {
    const void* q;
    const void* k;          // bytes
    const void* v;
    const int64_t* mask;    // [B, S] or NULL (MASKED = false)
    void* out;
    float* ws;              // [splits][B * nH][258], SPLIT only
    int64_t ldq;
    int nH, S;
    int range_keys;         // T * 64
    int ranges;             // the grid's y
    int rows;               // B * nH
    const float* k_scale;   // [B, nH]
    const float* v_scale;
    const int64_t* live;    // [B] or NULL (LIVE = false)
};

template <int CTRL>
__device__ __forceinline__ float kv8d_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// the sum over the 16 lanes of a DPP row, the same bits in each of them
__device__ __forceinline__ float kv8d_row_sum(float v) {
    v += kv8d_dpp<0x128>(v);   // row_ror:8
    v += kv8d_dpp<0x124>(v);   // row_ror:4
    v += kv8d_dpp<0x122>(v);   // row_ror:2
    return v + kv8d_dpp<0x121>(v);   // row_ror:1
}

__device__ __forceinline__ void kv8d_unpack(const vec4u& v, float (&f)[16]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(int(w[i]), false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(int(w[i]), true);
        f[4 * i] = lo[0];
        f[4 * i + 1] = lo[1];
        f[4 * i + 2] = hi[0];
        f[4 * i + 3] = hi[1];
    }
}

// o * vs / L; no live key at all: zeros.  A NaN L stays NaN.
__device__ __forceinline__ void kv8d_finish(float L, float vs, float& o0, float& o1) {
    const bool any = L > 0.f || L != L;
    o0 = any ? (o0 * vs) / L : 0.f;
    o1 = any ? (o1 * vs) / L : 0.f;
}

// blockIdx.x = b * nH + h, blockIdx.y = the key range.
template <bool MASKED, bool LIVE, bool SPLIT>
__global__ __launch_bounds__(kT5RowThreads) void k_t5_decode_attn_kv8_d256(const T5AttnKv8D256Args a) {
    constexpr int DKV = kKv8dDkv, EPV = kKv8dEpv, NF = kKv8dFlight;
    constexpr int LPR = Kv8dGeom::LPR, KPW = Kv8dGeom::KPW, NG = Kv8dGeom::NG;
    __shared__ float s_acc[NG * DKV];
    __shared__ float s_m[NG];
    __shared__ float s_l[NG];

    const int bh = blockIdx.x;
    const int b = bh / a.nH, h = bh - b * a.nH;
    if constexpr (LIVE) {
        if (a.live[b] == 0) {   // block-uniform; with a split the merge writes the zeros
            if constexpr (!SPLIT) t5_zero_row<uint16_t, DKV>(a.out, int64_t(bh) * DKV);
            return;
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int sl = lane % LPR;
    const int gg = wave * KPW + lane / LPR;
    const float ks = a.k_scale[bh];

    float qf[EPV];
    {
        const uint16_t* qp = static_cast<const uint16_t*>(a.q) + int64_t(b) * a.ldq + h * DKV + sl * EPV;
        float lo[8], hi[8];
        BF16T::unpack(*reinterpret_cast<const vec4u*>(qp), lo);
        BF16T::unpack(*reinterpret_cast<const vec4u*>(qp + 8), hi);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            qf[e] = lo[e];
            qf[8 + e] = hi[e];
        }
    }
    const int64_t base = int64_t(bh) * a.S * DKV + sl * EPV;   // bytes
    const uint8_t* K = static_cast<const uint8_t*>(a.k) + base;
    const uint8_t* V = static_cast<const uint8_t*>(a.v) + base;
    const int64_t* mask = MASKED ? a.mask + int64_t(b) * a.S : nullptr;

    float m = -INFINITY, l = 0.f, acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.f;

    const int begin = SPLIT ? int(blockIdx.y) * a.range_keys : 0;
    const int end = SPLIT ? min(a.S, begin + a.range_keys) : a.S;
#pragma unroll 1
    for (int j0 = begin + gg; j0 < end; j0 += kKv8dTrip) {
        bool on[NF], any = false;
        vec4u kk[NF], vv[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int j = j0 + f * NG;
            on[f] = j < end;
            if (MASKED) on[f] = on[f] && mask[on[f] ? j : j0] != 0;
            any = any || on[f];
            kk[f] = vec4u_make(0, 0, 0, 0);
            vv[f] = kk[f];
            if (on[f]) {
                kk[f] = *reinterpret_cast<const vec4u*>(K + int64_t(j) * DKV);
                vv[f] = *reinterpret_cast<const vec4u*>(V + int64_t(j) * DKV);
            }
        }
        if (!any) continue;   // uniform over the lane group: its 16 lanes share j0 and the mask words
        float s[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            float kf[EPV];
            kv8d_unpack(kk[f], kf);
            s[f] = 0.f;
#pragma unroll
            for (int e = 0; e < EPV; ++e) s[f] = fmaf(qf[e], kf[e], s[f]);
        }
        // the reduction needs every lane of the row: no lane of a group with a live key has left
        float mn = m;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            s[f] = kv8d_row_sum(s[f]) * ks;
            mn = on[f] ? fmaxf(mn, s[f]) : mn;
        }
        // a NaN score (a NaN scale) leaves mn at -inf on the first block: sc = exp(-inf + inf) = NaN, as it must
        const float sc = expf(m - mn);
        float p[NF], ps = 0.f;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            p[f] = on[f] ? expf(s[f] - mn) : 0.f;
            ps += p[f];
        }
        l = fmaf(l, sc, ps);
#pragma unroll
        for (int e = 0; e < EPV; ++e) acc[e] *= sc;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            float vf[EPV];
            kv8d_unpack(vv[f], vf);   // a masked key's vector is zero bytes and its p is 0
#pragma unroll
            for (int e = 0; e < EPV; ++e) acc[e] = fmaf(p[f], vf[e], acc[e]);
        }
        m = mn;
    }

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
            if (s_l[g] == 0.f) continue;   // no live key; a NaN l is not skipped
            const float w = expf(s_m[g] - M);
            L = fmaf(s_l[g], w, L);
            o0 = fmaf(s_acc[g * DKV + d], w, o0);
            o1 = fmaf(s_acc[g * DKV + d + 1], w, o1);
        }
        if constexpr (SPLIT) {
            float* rec = a.ws + (int64_t(blockIdx.y) * a.rows + bh) * kKv8dRec;
            if (threadIdx.x == 0) *reinterpret_cast<float2*>(rec) = make_float2(M, L);
            *reinterpret_cast<float2*>(rec + 2 + d) = make_float2(o0, o1);
        } else {
            kv8d_finish(L, a.v_scale[bh], o0, o1);
            t5_store_pair<uint16_t>(a.out, int64_t(bh) * DKV + d, o0, o1);
        }
    }
}

// Thread t of the grid: outputs d, d + 1 of (row, head) = t / 128, the ranges in split order.
template <bool LIVE>
__global__ __launch_bounds__(kT5RowThreads) void k_t5_decode_attn_kv8_d256_merge(const T5AttnKv8D256Args a) {
    constexpr int DKV = kKv8dDkv;
    const int64_t t = int64_t(blockIdx.x) * kT5RowThreads + threadIdx.x;
    const int64_t bh = t / (DKV / 2);
    if (bh >= a.rows) return;
    const int d = 2 * int(t - bh * (DKV / 2));
    float o0 = 0.f, o1 = 0.f;
    bool dead = false;
    if constexpr (LIVE) dead = a.live[bh / a.nH] == 0;
    if (!dead) {   // a dead row's states were not written and are not read
        const float* rec = a.ws + bh * kKv8dRec;
        const int64_t step = int64_t(a.rows) * kKv8dRec;
        float M = rec[0];
        for (int x = 1; x < a.ranges; ++x) M = fmaxf(M, rec[x * step]);
        float L = 0.f;
        for (int x = 0; x < a.ranges; ++x) {
            const float2 ml = *reinterpret_cast<const float2*>(rec + x * step);
            if (ml.y == 0.f) continue;   // a range with no live key
            const float2 o = *reinterpret_cast<const float2*>(rec + x * step + 2 + d);
            const float w = expf(ml.x - M);
            L = fmaf(ml.y, w, L);
            o0 = fmaf(o.x, w, o0);
            o1 = fmaf(o.y, w, o1);
        }
        kv8d_finish(L, a.v_scale[bh], o0, o1);
    }
    t5_store_pair<uint16_t>(a.out, bh * DKV + d, o0, o1);
}

typedef void (*t5_kv8d_kernel_t)(const T5AttnKv8D256Args);
template <bool SPLIT>
static t5_kv8d_kernel_t t5_pick_kv8d(bool masked, bool live) {
    if (live) return masked ? k_t5_decode_attn_kv8_d256<true, true, SPLIT> : k_t5_decode_attn_kv8_d256<false, true, SPLIT>;
    return masked ? k_t5_decode_attn_kv8_d256<true, false, SPLIT> : k_t5_decode_attn_kv8_d256<false, false, SPLIT>;
}

// whole trips a range: ceil(ceil(S / 64) / splits)
static int64_t t5_kv8d_range_keys(int64_t S, int64_t splits) {
    const int64_t ntrip = (S + kKv8dTrip - 1) / kKv8dTrip;
    return (ntrip + splits - 1) / splits * kKv8dTrip;
}

}  // namespace trlx

using namespace trlx;

extern "C" int64_t trlx_t5_decode_attn_kv8_d256_workspace_bytes(int64_t B, int64_t n_heads, int64_t splits) {
    if (B < 1 || n_heads < 1 || splits < 1 || splits > kKv8dMaxSplits) return 0;
    if (B > 0x7fffffffLL || n_heads > 0x7fffffffLL / 128 || B * n_heads > 0x7fffffffLL) return 0;
    return splits * B * n_heads * kKv8dRec * int64_t(sizeof(float));
}

extern "C" int trlx_t5_decode_attn_kv8_d256_geometry(int64_t S, int64_t splits, TrlxT5DecodeAttnKv8D256Geometry* g) {
    TRLX_REQUIRE(g, TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256, geometry: NULL result");
    *g = TrlxT5DecodeAttnKv8D256Geometry{};
    TRLX_REQUIRE(S >= 1 && S <= 0x7fffffffLL / 128, TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256, geometry: S %lld",
                 (long long)S);
    TRLX_REQUIRE(splits >= 1 && splits <= kKv8dMaxSplits, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys, d_kv 256, geometry: splits %lld (1 to %d)", (long long)splits, kKv8dMaxSplits);
    g->rows_per_wave_load = Kv8dGeom::KPW;
    g->lane_groups = Kv8dGeom::NG;
    g->keys_per_trip = kKv8dTrip;
    g->keys_per_range = t5_kv8d_range_keys(S, splits);
    g->ranges = (S + g->keys_per_range - 1) / g->keys_per_range;
    g->max_splits = kKv8dMaxSplits;
    return TRLX_OK;
}

extern "C" int trlx_t5_decode_attn_kv8_d256(const TrlxT5DecodeAttnArgs* a, const float* k_scale, const float* v_scale,
                                            const int64_t* live, int splits, void* workspace, int64_t workspace_bytes,
                                            void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256: NULL arguments");
    TRLX_REQUIRE(a->mode == TRLX_T5_ATTN_CROSS, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys, d_kv 256: mode %d (the cross-attention only)", a->mode);
    TRLX_REQUIRE(a->dtype == TRLX_BF16, TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256: dtype %d (bf16 q and out only)",
                 a->dtype);
    TRLX_REQUIRE(k_scale && v_scale, TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256: NULL k_scale / v_scale");
    auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    TRLX_REQUIRE(!mis(k_scale, 3) && !mis(v_scale, 3), TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys, d_kv 256: the scales are not aligned to 4 bytes");
    TRLX_REQUIRE(!mis(live, 7), TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256: live is not aligned to 8 bytes");
    TRLX_REQUIRE(a->d_kv == kKv8dDkv, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys, d_kv 256: d_kv %lld (64 and 128: trlx_t5_decode_attn_kv8)", (long long)a->d_kv);
    TRLX_REQUIRE(a->B >= 1 && a->n_heads >= 1 && a->max_len >= 1 && a->B * a->n_heads <= 0x7fffffffLL &&
                     a->max_len <= 0x7fffffffLL / 128 && a->n_heads <= 0x7fffffffLL / 128,
                 TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256: B %lld, heads %lld, max_len %lld", (long long)a->B,
                 (long long)a->n_heads, (long long)a->max_len);
    TRLX_REQUIRE(a->q && a->k && a->v && a->out, TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256: NULL q / K / V / out");
    const int64_t inner = a->n_heads * a->d_kv;
    const int64_t ldq = a->B == 1 ? inner : a->ldq;   // a single row has no stride to speak of
    TRLX_REQUIRE(ldq >= inner && ldq % 8 == 0, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys, d_kv 256: q row stride %lld (>= heads * d_kv = %lld, whole 16-byte vectors)",
                 (long long)ldq, (long long)inner);
    TRLX_REQUIRE(!mis(a->q, 15) && !mis(a->k, 15) && !mis(a->v, 15) && !mis(a->out, 15), TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys, d_kv 256: q, K, V and out must be 16-byte aligned");
    TRLX_REQUIRE(!a->k_new && !a->v_new && !a->bias_by_distance, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys, d_kv 256: k_new / v_new / bias_by_distance are for the self-attention only");
    TRLX_REQUIRE(!mis(a->key_mask, 7), TRLX_ERR_ARG, "t5 decode attention, fp8 keys, d_kv 256: key_mask not aligned to 8 bytes");
    TRLX_REQUIRE(splits >= 1 && splits <= kKv8dMaxSplits, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys, d_kv 256: splits %d (1 to %d)", splits, kKv8dMaxSplits);
    if (splits > 1) {
        const int64_t need = trlx_t5_decode_attn_kv8_d256_workspace_bytes(a->B, a->n_heads, splits);
        TRLX_REQUIRE(workspace && !mis(workspace, 15) && workspace_bytes >= need, TRLX_ERR_ARG,
                     "t5 decode attention, fp8 keys, d_kv 256: workspace %p of %lld bytes (16-byte aligned, at least %lld "
                     "bytes for %d splits)", workspace, (long long)workspace_bytes, (long long)need, splits);
    }
    T5AttnKv8D256Args k = {};
    k.q = a->q;
    k.k = a->k;
    k.v = a->v;
    k.mask = a->key_mask;
    k.out = a->out;
    k.ws = static_cast<float*>(workspace);
    k.ldq = ldq;
    k.nH = int(a->n_heads);
    k.S = int(a->max_len);
    k.range_keys = int(t5_kv8d_range_keys(a->max_len, splits));
    k.ranges = int((a->max_len + k.range_keys - 1) / k.range_keys);   // the non-empty ones, <= splits
    k.rows = int(a->B * a->n_heads);
    k.k_scale = k_scale;
    k.v_scale = v_scale;
    k.live = live;
    const bool masked = a->key_mask != nullptr, has_live = live != nullptr;
    if (splits == 1) {
        hipLaunchKernelGGL(t5_pick_kv8d<false>(masked, has_live), dim3(unsigned(k.rows)), dim3(kT5RowThreads), 0,
                           (hipStream_t)stream, k);
        return check_launch("k_t5_decode_attn_kv8_d256");
    }
    hipLaunchKernelGGL(t5_pick_kv8d<true>(masked, has_live), dim3(unsigned(k.rows), unsigned(k.ranges)), dim3(kT5RowThreads), 0,
                       (hipStream_t)stream, k);
    const int rc = check_launch("k_t5_decode_attn_kv8_d256 (split)");
    if (rc != TRLX_OK) return rc;
    const int64_t threads = int64_t(k.rows) * (kKv8dDkv / 2);
    hipLaunchKernelGGL(has_live ? k_t5_decode_attn_kv8_d256_merge<true> : k_t5_decode_attn_kv8_d256_merge<false>,
                       dim3(unsigned((threads + kT5RowThreads - 1) / kT5RowThreads)), dim3(kT5RowThreads), 0,
                       (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn_kv8_d256_merge");
}
