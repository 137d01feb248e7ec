// T5 full-sequence attention forward at d_kv 256 (the UL2 head size): trlx_t5_attention's semantics
// (t5_attention.hip) in a kernel with its own register and LDS budget.  DESIGN §3 has the budget.
//
// Split.  One workgroup = 4 waves = one (batch row, head, block of kTa256QTile = 128 query rows),
// ONE WAVE PER SIMD (__launch_bounds__(256, 1)): a wave then has the SIMD's whole register file,
// 512 registers a lane.  A wave owns 32 query rows and keeps in registers, for the whole walk,
// their Q^T fragments (16 k-steps x 4 = 64), O^T for all 256 value columns (8 blocks x 16 = 128, the
// MFMA accumulators), the S^T tile (16 per 32 keys) and the next K/V tile on its way to LDS.
// Nobody else is resident on the SIMD to hide a stall, so the kernel hides its own: the global
// loads of tile t + 1 (4 x 16 B of K and 4 of V a thread at 32 keys) are issued right after the
// barrier that publishes tile t and land in registers under tile t's 32 MFMAs; they are first
// touched by the LDS stores at the top of the next trip.  __builtin_amdgcn_sched_barrier keeps the
// scheduler from hoisting a whole tile's LDS fragments at once (with 512 registers to fill it
// otherwise does, and spills).
//
// Orientation, keys and bias are the d 64 / 128 kernel's: S^T = K·Q^T on v_mfma_f32_32x32x16_bf16
// (query on the lane), P^T rounded to bf16 un-normalised is the B operand of O^T = V^T·P^T, V^T
// comes out of the row-major V tile through ds_read_b64_tr_b16; a wave-uniform 64-bit mask of the
// tile's live keys decides which rows are loaded (a dead row is zeros in LDS and is never read from
// memory), a tile without a live key is skipped, and under a key mask only the tiles between the
// batch row's first and last live key are walked.
//
// LDS.  A K or V row is 512 B.  K rows are 528 B apart (132 dwords = 4 mod 64 banks: the 16 lanes
// of a quarter-wave b128 pass read 16 rows at banks 4 r .. 4 r + 3, all 64 distinct), V rows 576 B
// (144 dwords = 16 mod 64: a half-wave pass of the transposed b64 read covers 4 rows x 16 banks).
// 32 keys: 32 x (528 + 576) = 35,328 B.  O^T is staged through the same bytes in two passes of 128
// value columns (128 rows x 272 B) and leaves as whole 16-byte row vectors.  KVT = 64 (70,656 B, O
// in one pass) is the candidate that was not shipped: four of its instantiations spill.
//
// LSE (trlx_t5_attention_fwd_lse): the lane that holds a query also stores lse = m + log(l), +inf for a
// query with no live key, once after the walk; the instantiations without the flag are unchanged.
#include <climits>

#include <type_traits>

#include "t5_attention.h"

namespace trlx {

constexpr int kTdThreads = 256;
constexpr int kTdD = 256;

template <int KVT, int FLAGS, bool LSE = false>
__global__ __launch_bounds__(kTdThreads, 1) void k_t5_attention_d256(const std::conditional_t<LSE, TaArgsLse, TaArgs> a) {
    constexpr bool BIAS = FLAGS & kTaBias, MASK = FLAGS & kTaMask, CAUSAL = FLAGS & kTaCausal;
    constexpr int QT = kTa256QTile;
    constexpr int CPR = kTdD / 8;                           // 16-byte chunks per row
    constexpr int NC = KVT * CPR / kTdThreads;              // chunks per thread and operand
    constexpr int KS = 2 * kTdD + 16;                       // K row stride in LDS, bytes: b128 row reads
    constexpr int VS = 2 * kTdD + 64;                       // V row stride: the transposed reads
    constexpr int KK = kTdD / 16;                           // k-steps of K·Q^T
    constexpr int DB = kTdD / 32;                           // 32-row blocks of O^T
    constexpr int NKB = KVT / 32;                           // 32-key blocks of a tile
    constexpr int kBytes = KVT * (KS + VS);
    constexpr int OP = QT * (2 * kTdD + 16) <= kBytes ? 1 : 2;   // passes of the staged O, by columns
    constexpr int OC = kTdD / OP;                           // value columns per pass
    constexpr int OS = 2 * OC + 16;                         // staged O row stride
    constexpr int BW = QT + KVT;                            // offsets (key - query) a tile can meet, rounded up
    constexpr float L2E = 1.4426950408889634f;
    static_assert(KVT == 32 || KVT == 64, "the live-key mask is one 64-bit ballot");
    static_assert(NC * kTdThreads == KVT * CPR && QT == 128 && BW <= kTdThreads, "tile geometry");
    static_assert(QT * OS <= kBytes && DB % OP == 0, "O is staged through the K/V tiles' LDS");
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
    __shared__ float s_bias[BW];
    __shared__ int s_lohi[2];
    unsigned char* sK = smem;
    unsigned char* sV = smem + KVT * KS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    int bid = blockIdx.x;
    const int qb = bid % a.nqb;
    bid /= a.nqb;
    const int h = bid % a.nH, b = bid / a.nH;
    const int q0 = qb * QT;
    const int qw0 = q0 + wave * 32;        // this wave's first query
    const int qg = qw0 + c;                // this lane's query
    const int qmax = min(q0 + QT - 1, a.Tq - 1);
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
    int t_lo = 0, t_hi = (kend + KVT - 1) / KVT;
    if (MASK) {
        if (tid == 0) {
            s_lohi[0] = INT_MAX;
            s_lohi[1] = -1;
        }
        __syncthreads();
        int lo = INT_MAX, hi = -1;
        for (int j = tid; j < kend; j += kTdThreads)
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
        t_lo = hi < 0 ? 0 : lo / KVT;
        t_hi = hi < 0 ? 0 : hi / KVT + 1;
    }

    // tile t into registers: the live-key mask, the live rows' K and V chunks, the bias window.  A
    // wave's 64 lanes take two whole 512-byte rows per chunk index.
    static_assert(CPR == 32 && kTdThreads / CPR == 8, "a half-wave a row, 8 rows a chunk index");
    const uint16_t* klane = kbase + int64_t(hh) * a.k_st + c * 8;
    const uint16_t* vlane = vbase + int64_t(hh) * a.v_st + c * 8;
    vec4u kr[NC], vr[NC];
    float br = 0.f;
    unsigned long long lmN = 0;
    auto prefetch = [&](int t) __attribute__((always_inline)) {
        const int k0 = t * KVT;
        const int key = k0 + lane;
        bool live = lane < KVT && key < kend;
        if (MASK) live = live && mrow[live ? key : 0] != 0;
        lmN = __ballot(live);
#pragma unroll
        for (int n = 0; n < NC; ++n) {   // row 2 wave + 8 n + (lane >> 5) of the tile: a uniform part and the lane's
            const int ur = 2 * wave + 8 * n;
            kr[n] = vec4u_make(0, 0, 0, 0);
            vr[n] = kr[n];
            if ((lmN >> (ur + hh)) & 1) {
                kr[n] = *reinterpret_cast<const vec4u*>(klane + int64_t(k0 + ur) * a.k_st);
                vr[n] = *reinterpret_cast<const vec4u*>(vlane + int64_t(k0 + ur) * a.v_st);
            }
        }
        if (BIAS && tid < BW) {   // entry e is the offset (key - query) = k0 - (q0 + 127) + e
            const int idx = k0 - q0 - (QT - 1) + (a.Tq - 1) + tid;
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
        const int k0 = t * KVT;
        if (lm) {
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int cid = tid + kTdThreads * n;
                const int row = cid / CPR, ch = cid % CPR;
                *reinterpret_cast<vec4u*>(sK + row * KS + ch * 16) = kr[n];
                *reinterpret_cast<vec4u*>(sV + row * VS + ch * 16) = vr[n];
            }
            if (BIAS && tid < BW) s_bias[tid] = br;
        }
        __syncthreads();
        if (t + 1 < t_hi) prefetch(t + 1);   // in flight under the MFMAs below

        const bool active = lm != 0 && wave_live && (!CAUSAL || k0 <= min(qw0 + 31, a.Tq - 1));
        if (active) {
            // S^T = K·Q^T, NKB blocks of 32 keys
            ta_f32x16 sacc[NKB];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
                const unsigned char* kp = sK + (32 * kb + c) * KS + 16 * hh;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const ta_bf16x8 kf = *reinterpret_cast<const ta_bf16x8*>(kp + 32 * kk);
                    sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], sacc[kb], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);   // one block's K fragments live at a time
            }
            // bias, dead keys, the causal rule; the tile's max per query
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                const uint32_t w = uint32_t(lm >> (32 * kb)) >> (4 * hh);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int kl0 = (i & 3) + 8 * (i >> 2);        // key in the block, less 4 hh
                    const int kl = 32 * kb + kl0 + 4 * hh;         // key in the tile
                    float s = sacc[kb][i];
                    if (BIAS) s += s_bias[kl - (wave * 32 + c) + (QT - 1)];
                    bool dead = !((w >> kl0) & 1u);
                    if (CAUSAL) dead = dead || k0 + kl > qg;
                    s = dead ? -INFINITY : s;
                    sacc[kb][i] = s;
                    mx = fmaxf(mx, s);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
            const float mn = fmaxf(m, mx);
            const float mu = mn == -INFINITY ? 0.f : mn;   // no live key yet: every p is exp2(-inf) = 0
            const float sc = exp2_fast((m - mu) * L2E);
            m = mn;
            float ps = 0.f;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = exp2_fast((sacc[kb][i] - mu) * L2E);
                    sacc[kb][i] = p;
                    ps += p;
                }
            l = l * sc + ps;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) O[db][i] *= sc;
            __builtin_amdgcn_sched_barrier(0);
            // O^T += V^T·P^T, V^T through the transposed read (ta_tr_base / ta_tr_frag)
            const unsigned char* vp = ta_tr_base(sV, VS, lane);
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    ta_bf16x8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = static_cast<__bf16>(sacc[kb][8 * s + j]);
#pragma unroll
                    for (int db = 0; db < DB; ++db) {
                        const ta_bf16x8 vf = ta_tr_frag(vp + (32 * kb + 16 * s) * VS + 64 * db, VS);
                        O[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, O[db], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);   // one k-step's V^T fragments live at a time
                }
        }
        __syncthreads();
    }

    // normalise, round once, stage the wave's 32 rows in LDS (OC columns a pass) and store whole rows
    l += __shfl_xor(l, 32, kWave);
    const bool any = l > 0.f || l != l;   // no live key at all: zeros
    if constexpr (LSE) {   // m + log(l), what the backward rebuilds P from; +inf makes its exp(s - lse) zero
        if (hh == 0 && qg < a.Tq) a.lse[(int64_t(b) * a.nH + h) * a.Tq + qg] = any ? m + logf(l) : INFINITY;
    }
    const float rl = any ? l : 1.f;
    unsigned char* sO = smem + wave * 32 * OS;
    uint16_t* obase = a.out + int64_t(b) * a.o_sb + int64_t(h) * a.o_sh;
#pragma unroll
    for (int p = 0; p < OP; ++p) {
        if (p) __syncthreads();
#pragma unroll
        for (int dbl = 0; dbl < DB / OP; ++dbl)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = any ? O[p * (DB / OP) + dbl][4 * g + e] / rl : 0.f;
                uint2 pk;
                pk.x = pack_bf2(o[0], o[1]);
                pk.y = pack_bf2(o[2], o[3]);
                *reinterpret_cast<uint2*>(sO + c * OS + (32 * dbl + 8 * g + 4 * hh) * 2) = pk;
                __builtin_amdgcn_sched_barrier(0);
            }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 32 * (OC / 8) / kWave; ++n) {
            const int cid = lane + kWave * n;
            const int row = cid / (OC / 8), ch = cid % (OC / 8);
            if (qw0 + row < a.Tq)
                *reinterpret_cast<vec4u*>(obase + int64_t(qw0 + row) * a.o_st + p * OC + ch * 8) =
                    *reinterpret_cast<const vec4u*>(sO + row * OS + ch * 16);
        }
    }
}

template <bool LSE>
static auto ta256_pick(int flags) -> void (*)(const std::conditional_t<LSE, TaArgsLse, TaArgs>) {
    switch (flags) {
        case 0: return k_t5_attention_d256<kTa256KVTile, 0, LSE>;
        case 1: return k_t5_attention_d256<kTa256KVTile, 1, LSE>;
        case 2: return k_t5_attention_d256<kTa256KVTile, 2, LSE>;
        case 3: return k_t5_attention_d256<kTa256KVTile, 3, LSE>;
        case 4: return k_t5_attention_d256<kTa256KVTile, 4, LSE>;
        case 5: return k_t5_attention_d256<kTa256KVTile, 5, LSE>;
        case 6: return k_t5_attention_d256<kTa256KVTile, 6, LSE>;
        default: return k_t5_attention_d256<kTa256KVTile, 7, LSE>;
    }
}

int ta_launch_d256(const TaArgs& k, int flags, unsigned grid, float* lse, void* stream) {
    if (lse) {
        TaArgsLse kl;
        static_cast<TaArgs&>(kl) = k;
        kl.lse = lse;
        hipLaunchKernelGGL(ta256_pick<true>(flags), dim3(grid), dim3(kTdThreads), 0, (hipStream_t)stream, kl);
    } else {
        hipLaunchKernelGGL(ta256_pick<false>(flags), dim3(grid), dim3(kTdThreads), 0, (hipStream_t)stream, k);
    }
    return check_launch("k_t5_attention_d256");
}

}  // namespace trlx
