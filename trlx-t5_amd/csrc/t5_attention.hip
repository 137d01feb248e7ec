// T5 full-sequence attention forward (many queries x many keys) with the relative-position bias,
// the key mask and the causal rule inside one launch.  See trlx_t5_attention in trlx_t5_amd.h.
//
// Flash-attention forward on v_mfma_f32_32x32x16_bf16.  One workgroup = 4 waves = one (batch row,
// head, block of kTaQTile = 128 query rows); a wave owns 32 query rows and keeps their Q fragments,
// their running max / sum and O^T in registers.  K/V tiles of kTaKVTile = 64 keys go global ->
// registers (issued one tile ahead, under the MFMAs of the current tile) -> LDS, shared by the waves.
//
// Orientation.  Scores are computed transposed, S^T = K·Q^T (A = K rows, B = Q^T), so a 32x32
// result has its QUERY on the lane (lane & 31) and 16 of the 32 keys in the lane's registers
// (key = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)); the other 16 sit in lane ^ 32.  The softmax state of
// a query is then lane-local but for one exchange with lane ^ 32 per tile.  P^T rounded to bf16 is
// directly the B operand of O^T = V^T·P^T (registers 8s .. 8s+7 are k-step s, no lane movement); the
// A operand V^T comes out of the row-major V tile through ds_read_b64_tr_b16 in the same permuted
// key order.  O^T has the query on the lane again, so the rescale is one factor per lane.
//
// Keys.  A wave-uniform 64-bit mask of the tile's live keys (in range, key_mask != 0) decides what
// is loaded: a dead row is neither read nor left as it is (its LDS row is zeros, so a NaN there
// cannot reach an MFMA); a tile without a live key is skipped whole.  With a key mask the
// workgroup first finds the first and the last live key of its batch row and walks only the tiles
// between them.  Causal: tiles wholly above the workgroup's last query are not walked, a wave
// skips the tiles above its own last query.
#include <climits>

#include <type_traits>

#include "t5_attention.h"

namespace trlx {

constexpr int kTaThreads = 256;
constexpr int kTaQTile = 128;   // query rows per workgroup (32 per wave)
constexpr int kTaKVTile = 64;   // keys per LDS tile
constexpr int kTaBiasWin = kTaQTile + kTaKVTile;   // offsets (key - query) a tile can meet, rounded up

struct TaArgs {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    uint16_t* out;
    const float* bias;     // [nH, Tq + S - 1] or NULL
    const int64_t* mask;   // [B, S] or NULL
    int64_t q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh;
    int nH, Tq, S, nqb;
};

// the same arguments plus the row statistics' destination (trlx_t5_attention_fwd_lse)
struct TaArgsLse : TaArgs {
    float* lse;            // [B, nH, Tq] fp32
};

template <int DKV, int FLAGS, bool LSE = false>
__global__ __launch_bounds__(kTaThreads, 2) void k_t5_attention(const std::conditional_t<LSE, TaArgsLse, TaArgs> a) {
    constexpr bool BIAS = FLAGS & kTaBias, MASK = FLAGS & kTaMask, CAUSAL = FLAGS & kTaCausal;
    constexpr int CPR = DKV / 8;                            // 16-byte chunks per row
    constexpr int NC = kTaKVTile * CPR / kTaThreads;        // chunks per thread and operand
    constexpr int KS = 2 * DKV + 16;                        // K row stride in LDS, bytes: b128 row reads
    constexpr int VS = 2 * DKV + 64;                        // V row stride: the transposed reads
    constexpr int OS = 2 * DKV + 16;                        // staged O row stride
    constexpr int KK = DKV / 16;                            // k-steps of K·Q^T
    constexpr int DB = DKV / 32;                            // 32-row blocks of O^T
    constexpr int kBytes = kTaKVTile * (KS + VS);
    constexpr float L2E = 1.4426950408889634f;
    static_assert(kTaQTile * OS <= kBytes, "O is staged through the K/V tiles' LDS");
    static_assert(NC * kTaThreads == kTaKVTile * CPR && kTaKVTile == 64 && kTaQTile == 128, "tile geometry");
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
    __shared__ float s_bias[kTaBiasWin];
    __shared__ int s_lohi[2];
    unsigned char* sK = smem;
    unsigned char* sV = smem + kTaKVTile * KS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    int bid = blockIdx.x;
    const int qb = bid % a.nqb;
    bid /= a.nqb;
    const int h = bid % a.nH, b = bid / a.nH;
    const int q0 = qb * kTaQTile;
    const int qw0 = q0 + wave * 32;        // this wave's first query
    const int qg = qw0 + c;                // this lane's query
    const int qmax = min(q0 + kTaQTile - 1, a.Tq - 1);
    const bool wave_live = qw0 < a.Tq;

    // Q^T fragments: lane (c, hh) holds Q[query c][d = 16 kk + 8 hh + 0..7]; rows past Tq are clamped
    ta_bf16x8 qf[KK];
    {
        const uint16_t* qp = a.q + int64_t(b) * a.q_sb + int64_t(min(qg, a.Tq - 1)) * a.q_st + int64_t(h) * a.q_sh + 8 * hh;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) qf[kk] = *reinterpret_cast<const ta_bf16x8*>(qp + 16 * kk);
    }
    const uint16_t* kbase = a.k + int64_t(b) * a.k_sb + int64_t(h) * a.k_sh;
    const uint16_t* vbase = a.v + int64_t(b) * a.v_sb + int64_t(h) * a.v_sh;
    const float* brow = BIAS ? a.bias + int64_t(h) * (a.Tq + a.S - 1) : nullptr;
    const int64_t* mrow = MASK ? a.mask + int64_t(b) * a.S : nullptr;

    // keys [0, kend) can matter to this workgroup; the tiles walked are [t_lo, t_hi)
    const int kend = CAUSAL ? min(a.S, qmax + 1) : a.S;
    int t_lo = 0, t_hi = (kend + kTaKVTile - 1) / kTaKVTile;
    if (MASK) {
        if (tid == 0) {
            s_lohi[0] = INT_MAX;
            s_lohi[1] = -1;
        }
        __syncthreads();
        int lo = INT_MAX, hi = -1;
        for (int j = tid; j < kend; j += kTaThreads)
            if (mrow[j] != 0) {
                lo = min(lo, j);
                hi = j;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = min(lo, __shfl_xor(lo, off, kWave));
            hi = max(hi, __shfl_xor(hi, off, kWave));
        }
        if (lane == 0) {
            atomicMin(&s_lohi[0], lo);
            atomicMax(&s_lohi[1], hi);
        }
        __syncthreads();
        lo = s_lohi[0];
        hi = s_lohi[1];
        t_lo = hi < 0 ? 0 : lo / kTaKVTile;
        t_hi = hi < 0 ? 0 : hi / kTaKVTile + 1;
    }

    // tile t into registers: the live-key mask, the live rows' K and V chunks, the bias window
    vec4u kr[NC], vr[NC];
    float br = 0.f;
    unsigned long long lmN = 0;
    auto prefetch = [&](int t) __attribute__((always_inline)) {
        const int k0 = t * kTaKVTile;
        const int key = k0 + lane;
        bool live = key < kend;
        if (MASK) live = live && mrow[live ? key : 0] != 0;
        lmN = __ballot(live);
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const int cid = tid + kTaThreads * n;
            const int row = cid / CPR, ch = cid % CPR;
            kr[n] = vec4u_make(0, 0, 0, 0);
            vr[n] = kr[n];
            if ((lmN >> row) & 1) {
                kr[n] = *reinterpret_cast<const vec4u*>(kbase + int64_t(k0 + row) * a.k_st + ch * 8);
                vr[n] = *reinterpret_cast<const vec4u*>(vbase + int64_t(k0 + row) * a.v_st + ch * 8);
            }
        }
        if (BIAS && tid < kTaBiasWin) {   // entry e is the offset (key - query) = k0 - (q0 + 127) + e
            const int idx = k0 - q0 - (kTaQTile - 1) + (a.Tq - 1) + tid;
            br = idx >= 0 && idx < a.Tq + a.S - 1 ? brow[idx] : 0.f;
        }
    };

    float m = -INFINITY, l = 0.f;
    ta_f32x16 O[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) O[db][i] = 0.f;

    if (t_lo < t_hi) prefetch(t_lo);
#pragma unroll 1
    for (int t = t_lo; t < t_hi; ++t) {
        const unsigned long long lm = lmN;
        const int k0 = t * kTaKVTile;
        if (lm) {
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int cid = tid + kTaThreads * n;
                const int row = cid / CPR, ch = cid % CPR;
                *reinterpret_cast<vec4u*>(sK + row * KS + ch * 16) = kr[n];
                *reinterpret_cast<vec4u*>(sV + row * VS + ch * 16) = vr[n];
            }
            if (BIAS && tid < kTaBiasWin) s_bias[tid] = br;
        }
        __syncthreads();
        if (t + 1 < t_hi) prefetch(t + 1);

        const bool active = lm != 0 && wave_live && (!CAUSAL || k0 <= min(qw0 + 31, a.Tq - 1));
        if (active) {
            // S^T = K·Q^T, two blocks of 32 keys
            ta_f32x16 sacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
                const unsigned char* kp = sK + (32 * kb + c) * KS + 16 * hh;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const ta_bf16x8 kf = *reinterpret_cast<const ta_bf16x8*>(kp + 32 * kk);
                    sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], sacc[kb], 0, 0, 0);
                }
            }
            // bias, dead keys, the causal rule; the tile's max per query
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const uint32_t w = uint32_t(lm >> (32 * kb)) >> (4 * hh);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int kl0 = (i & 3) + 8 * (i >> 2);        // key in the block, less 4 hh
                    const int kl = 32 * kb + kl0 + 4 * hh;         // key in the tile
                    float s = sacc[kb][i];
                    if (BIAS) s += s_bias[kl - (wave * 32 + c) + (kTaQTile - 1)];
                    bool dead = !((w >> kl0) & 1u);
                    if (CAUSAL) dead = dead || k0 + kl > qg;
                    s = dead ? -INFINITY : s;
                    sacc[kb][i] = s;
                    mx = fmaxf(mx, s);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
            const float mn = fmaxf(m, mx);
            const float mu = mn == -INFINITY ? 0.f : mn;   // no live key yet: every p is exp2(-inf) = 0
            const float sc = exp2_fast((m - mu) * L2E);
            m = mn;
            float ps = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = exp2_fast((sacc[kb][i] - mu) * L2E);
                    sacc[kb][i] = p;
                    ps += p;
                }
            l = l * sc + ps;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) O[db][i] *= sc;
            // O^T += V^T·P^T.  Lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3 of
            // a 4-key x 16-column block of V and receives its column (lane & 15) of the 4 keys.
            const unsigned char* vp = sV + (4 * hh + ((lane & 15) >> 2)) * VS + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    ta_bf16x8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = static_cast<__bf16>(sacc[kb][8 * s + j]);
#pragma unroll
                    for (int db = 0; db < DB; ++db) {
                        const unsigned char* p0 = vp + (32 * kb + 16 * s) * VS + 64 * db;
                        const ta_s16x4 v0 = ta_tr_read(p0), v1 = ta_tr_read(p0 + 8 * VS);
                        const ta_bf16x8 vf = __builtin_bit_cast(
                            ta_bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
                        O[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, O[db], 0, 0, 0);
                    }
                }
        }
        __syncthreads();
    }

    // normalise, round once, stage the wave's 32 rows in LDS and store whole rows
    l += __shfl_xor(l, 32, kWave);
    const bool any = l > 0.f || l != l;   // no live key at all: zeros
    if constexpr (LSE) {   // m + log(l), what the backward rebuilds P from; +inf makes its exp(s - lse) zero
        if (hh == 0 && qg < a.Tq) a.lse[(int64_t(b) * a.nH + h) * a.Tq + qg] = any ? m + logf(l) : INFINITY;
    }
    unsigned char* sO = smem + wave * 32 * OS;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = any ? O[db][4 * g + e] / l : 0.f;
            uint2 pk;
            pk.x = pack_bf2(o[0], o[1]);
            pk.y = pack_bf2(o[2], o[3]);
            *reinterpret_cast<uint2*>(sO + c * OS + (32 * db + 8 * g + 4 * hh) * 2) = pk;
        }
    __syncthreads();
    uint16_t* obase = a.out + int64_t(b) * a.o_sb + int64_t(h) * a.o_sh;
#pragma unroll
    for (int n = 0; n < 32 * CPR / kWave; ++n) {
        const int cid = lane + kWave * n;
        const int row = cid / CPR, ch = cid % CPR;
        if (qw0 + row < a.Tq)
            *reinterpret_cast<vec4u*>(obase + int64_t(qw0 + row) * a.o_st + ch * 8) =
                *reinterpret_cast<const vec4u*>(sO + row * OS + ch * 16);
    }
}

template <int DKV, bool LSE>
static auto ta_pick_flags(int flags) -> void (*)(const std::conditional_t<LSE, TaArgsLse, TaArgs>) {
    switch (flags) {
        case 0: return k_t5_attention<DKV, 0, LSE>;
        case 1: return k_t5_attention<DKV, 1, LSE>;
        case 2: return k_t5_attention<DKV, 2, LSE>;
        case 3: return k_t5_attention<DKV, 3, LSE>;
        case 4: return k_t5_attention<DKV, 4, LSE>;
        case 5: return k_t5_attention<DKV, 5, LSE>;
        case 6: return k_t5_attention<DKV, 6, LSE>;
        default: return k_t5_attention<DKV, 7, LSE>;
    }
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_attention_tiles(int* q_tile, int* kv_tile) {
    if (q_tile) *q_tile = kTaQTile;
    if (kv_tile) *kv_tile = kTaKVTile;
    return TRLX_OK;
}

// the checks and the launch of both entries; with_lse picks the instantiations that also write lse
static int ta_forward(const TrlxT5AttentionArgs* a, float* lse, bool with_lse, void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 attention: NULL arguments");
    TRLX_REQUIRE(!with_lse || (lse && (reinterpret_cast<uintptr_t>(lse) & 3u) == 0), TRLX_ERR_ARG,
                 "t5 attention: lse is NULL or not aligned to 4 bytes");
    TRLX_REQUIRE(a->dtype == TRLX_BF16, TRLX_ERR_ARG, "t5 attention: dtype %d (bf16 only)", a->dtype);
    TRLX_REQUIRE(a->d_kv == 64 || a->d_kv == 128, TRLX_ERR_ARG, "t5 attention: d_kv %lld (64 and 128 only)",
                 (long long)a->d_kv);
    const int64_t lim = int64_t(1) << 30;
    TRLX_REQUIRE(a->B >= 1 && a->n_heads >= 1 && a->Tq >= 1 && a->S >= 1 && a->B <= lim && a->n_heads <= lim &&
                     a->Tq <= lim && a->S <= lim,
                 TRLX_ERR_ARG, "t5 attention: B %lld, heads %lld, Tq %lld, S %lld (each in [1, 2^30])", (long long)a->B,
                 (long long)a->n_heads, (long long)a->Tq, (long long)a->S);
    const int64_t nqb = (a->Tq + kTaQTile - 1) / kTaQTile;
    int64_t grid;
    TRLX_REQUIRE(!__builtin_mul_overflow(a->B, a->n_heads, &grid) && !__builtin_mul_overflow(grid, nqb, &grid) &&
                     grid <= 0x7fffffffLL,
                 TRLX_ERR_ARG, "t5 attention: B * heads * query blocks = %lld * %lld * %lld exceeds the grid",
                 (long long)a->B, (long long)a->n_heads, (long long)nqb);
    TRLX_REQUIRE(!a->causal || a->Tq == a->S, TRLX_ERR_ARG, "t5 attention: causal needs Tq == S, got %lld and %lld",
                 (long long)a->Tq, (long long)a->S);
    TRLX_REQUIRE(a->q && a->k && a->v && a->out, TRLX_ERR_ARG, "t5 attention: NULL q / k / v / out");
    TRLX_REQUIRE(ta_aligned16(a->q) && ta_aligned16(a->k) && ta_aligned16(a->v) && ta_aligned16(a->out), TRLX_ERR_ARG,
                 "t5 attention: q, k, v and out must be 16-byte aligned");
    int64_t span;
    TRLX_REQUIRE(ta_strides_ok(a->B, a->Tq, a->n_heads, a->d_kv, a->q_stride_b, a->q_stride_t, a->q_stride_h, false, &span),
                 TRLX_ERR_ARG, "t5 attention: q strides %lld / %lld / %lld (multiples of 8, rows of d_kv apart)",
                 (long long)a->q_stride_b, (long long)a->q_stride_t, (long long)a->q_stride_h);
    TRLX_REQUIRE(ta_strides_ok(a->B, a->S, a->n_heads, a->d_kv, a->k_stride_b, a->k_stride_t, a->k_stride_h, false, &span),
                 TRLX_ERR_ARG, "t5 attention: k strides %lld / %lld / %lld (multiples of 8, rows of d_kv apart)",
                 (long long)a->k_stride_b, (long long)a->k_stride_t, (long long)a->k_stride_h);
    TRLX_REQUIRE(ta_strides_ok(a->B, a->S, a->n_heads, a->d_kv, a->v_stride_b, a->v_stride_t, a->v_stride_h, false, &span),
                 TRLX_ERR_ARG, "t5 attention: v strides %lld / %lld / %lld (multiples of 8, rows of d_kv apart)",
                 (long long)a->v_stride_b, (long long)a->v_stride_t, (long long)a->v_stride_h);
    TRLX_REQUIRE(ta_strides_ok(a->B, a->Tq, a->n_heads, a->d_kv, a->o_stride_b, a->o_stride_t, a->o_stride_h, true, &span),
                 TRLX_ERR_ARG, "t5 attention: out strides %lld / %lld / %lld (multiples of 8, rows that do not overlap)",
                 (long long)a->o_stride_b, (long long)a->o_stride_t, (long long)a->o_stride_h);
    TRLX_REQUIRE(!a->bias_by_offset || (reinterpret_cast<uintptr_t>(a->bias_by_offset) & 3u) == 0, TRLX_ERR_ARG,
                 "t5 attention: bias_by_offset not aligned to 4 bytes");
    TRLX_REQUIRE(!a->key_mask || (reinterpret_cast<uintptr_t>(a->key_mask) & 7u) == 0, TRLX_ERR_ARG,
                 "t5 attention: key_mask not aligned to 8 bytes");
    TaArgs k = {};
    k.q = static_cast<const uint16_t*>(a->q);
    k.k = static_cast<const uint16_t*>(a->k);
    k.v = static_cast<const uint16_t*>(a->v);
    k.out = static_cast<uint16_t*>(a->out);
    k.bias = a->bias_by_offset;
    k.mask = a->key_mask;
    // a stride that is never multiplied by a non-zero index is not read
    k.q_sb = a->B == 1 ? 0 : a->q_stride_b;
    k.q_st = a->Tq == 1 ? 0 : a->q_stride_t;
    k.q_sh = a->n_heads == 1 ? 0 : a->q_stride_h;
    k.k_sb = a->B == 1 ? 0 : a->k_stride_b;
    k.k_st = a->S == 1 ? 0 : a->k_stride_t;
    k.k_sh = a->n_heads == 1 ? 0 : a->k_stride_h;
    k.v_sb = a->B == 1 ? 0 : a->v_stride_b;
    k.v_st = a->S == 1 ? 0 : a->v_stride_t;
    k.v_sh = a->n_heads == 1 ? 0 : a->v_stride_h;
    k.o_sb = a->B == 1 ? 0 : a->o_stride_b;
    k.o_st = a->Tq == 1 ? 0 : a->o_stride_t;
    k.o_sh = a->n_heads == 1 ? 0 : a->o_stride_h;
    k.nH = int(a->n_heads);
    k.Tq = int(a->Tq);
    k.S = int(a->S);
    k.nqb = int(nqb);
    const int flags = (a->bias_by_offset ? kTaBias : 0) | (a->key_mask ? kTaMask : 0) | (a->causal ? kTaCausal : 0);
    if (with_lse) {
        TaArgsLse kl;
        static_cast<TaArgs&>(kl) = k;
        kl.lse = lse;
        auto fn = a->d_kv == 64 ? ta_pick_flags<64, true>(flags) : ta_pick_flags<128, true>(flags);
        hipLaunchKernelGGL(fn, dim3(unsigned(grid)), dim3(kTaThreads), 0, (hipStream_t)stream, kl);
    } else {
        auto fn = a->d_kv == 64 ? ta_pick_flags<64, false>(flags) : ta_pick_flags<128, false>(flags);
        hipLaunchKernelGGL(fn, dim3(unsigned(grid)), dim3(kTaThreads), 0, (hipStream_t)stream, k);
    }
    return check_launch("k_t5_attention");
}

extern "C" int trlx_t5_attention(const TrlxT5AttentionArgs* a, void* stream) {
    return ta_forward(a, nullptr, false, stream);
}

extern "C" int trlx_t5_attention_fwd_lse(const TrlxT5AttentionArgs* a, float* lse, void* stream) {
    return ta_forward(a, lse, true, stream);
}
