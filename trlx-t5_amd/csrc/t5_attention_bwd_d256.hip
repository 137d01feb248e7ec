// T5 full-sequence attention backward at d_kv 256 (the UL2 head size): the dk / dv and the dq kernels
// behind trlx_t5_attention_bwd, with register and LDS budgets of their own.  The semantics, the three
// launches and the delta kernel (k_t5_attn_bwd_delta<256>, the MFMA diagonal over 16 k-steps) are
// t5_attention_bwd.hip's; DESIGN §"T5 attention backward at d_kv 256" has the budgets.
//
// dq.  k_t5_attn_bwd_dq_d256: one workgroup = 4 waves = 128 queries of one (batch row, head), ONE WAVE
// PER SIMD (__launch_bounds__(256, 1)) as in the d 256 forward.  A wave owns 32 queries and keeps, for
// the whole walk, their Q^T and dO^T fragments (2 x 64 registers), dQ^T for all 256 columns (8 blocks
// x 16 = 128 accumulators), one S^T and one dP^T tile (32) and the next K/V tile on its way to LDS (32).
// Keys are walked in LDS tiles of 32; tile t + 1's global loads are issued right after the barrier
// that publishes tile t.  Orientation is the d 64 / 128 dq's on v_mfma_f32_32x32x16_bf16: S^T = K·Q^T and
// dP^T = V·dO^T with the query on the lane (lse and delta one value per lane), dS^T rounded to bf16 is
// the B operand of dQ^T = K^T·dS^T, K^T through ds_read_b64_tr_b16.  dP^T is summed over d in the 16
// k-steps the delta kernel takes, so a query with one live key has dS = 0 exactly.  dQ leaves through
// the tiles' LDS in two passes of 128 columns.  DBIAS: the LDS ring of 256 offsets; a 128 x 32 tile
// pair spans 160, the 32 that leave the window per step go out with global fp32 atomics.
// ORD: the ordered form of t5_attention_bwd.hip (a ring per half-wave, partial rows, no global atomic).
//
// dk / dv.  k_t5_attn_bwd_dkv_d256: one workgroup = 4 waves = 64 keys of one (batch row, head), a wave
// owns 16 keys, on v_mfma_f32_16x16x32_bf16: at 32 keys a wave dK^T and dV^T alone are 256
// accumulators and the kernel does not fit a lane's 512 registers.  At 16 keys: dK^T, dV^T [256 x 16]
// are 2 x 16 blocks x 4 = 128 accumulators, the wave's K and V fragments 2 x 8 k-steps x 4 = 64, S and
// dP for 32 queries 8 + 8.  Queries are walked in LDS tiles of 32 rows of Q and dO (global ->
// registers one tile ahead -> LDS).  S = Q·K^T and dP = dO·V^T: A = 16 query rows from LDS (lane
// (r, g) reads row r, d = 32 kk + 8 g + 0..7), B = the wave's fragments, so a 16 x 16 result has its
// KEY on the lane (lane & 15) and queries 4 g + 0..3 in the registers.  Two such results (queries
// 0..15 and 16..31) rounded to bf16 are, with no lane movement, the B operand of one k = 32 step of
// dV^T += dO^T·P and dK^T += Q^T·dS in the query order 4 g + 0..3, 16 + 4 g + 0..3; the A operands come
// out of the row-major dO and Q tiles in that order through two transposed reads (tb16_tr_frag).
// A chain of 8 k = 32 steps gives the bits of the delta kernel's chain of 16 k = 16 steps (both add
// 8-element partial sums to the accumulator in the order of d), which is what dS = 0 with one live
// key needs here too; tests/test_gpu_t5_attention_bwd_d256.py holds it at S = 1.
//
// LDS.  Rows are 512 B, 528 B apart (132 dwords = 4 mod 64 banks: the 16 rows of a quarter-wave's
// b128 row reads fall on 64 distinct banks).  dq: K tile 32 x 528, V tile 32 x 576 (the forward's
// strides), 35,328 B, restaged as 128 x 272 B of dQ per pass.  dkv: Q and dO tiles 32 x 528 each,
// 33,792 B, restaged as 4 x 16 rows x 528 B of dK, then dV.
#include <climits>

#include "t5_attention.h"

namespace trlx {

constexpr int kT2Threads = 256;
constexpr int kT2D = 256;
constexpr int kT2Ring = 256;      // dbias ring in LDS (a power of two)
constexpr int kT2Rings = 2 * kT2Threads / kWave;   // ordered dbias: a ring per (wave, half-wave)
constexpr float kT2L2E = 1.4426950408889634f;

typedef float tb_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ ta_bf16x8 tb2_zero_frag() { return __builtin_bit_cast(ta_bf16x8, vec4u_make(0, 0, 0, 0)); }

// The A operand of a 16x16x32 MFMA whose 16 rows are COLUMNS of a row-major LDS tile and whose 32
// k-indices are tile rows in the order 4 g + 0..3, 16 + 4 g + 0..3 for the lane group g = lane >> 4
// (the order two 16x16 results side by side have them in as a B operand).  Lane 4 q + p of a 16-lane
// group addresses row 4 g + q, columns 4 p .. 4 p + 3 of a 4-row x 16-column block and receives its
// column (lane & 15) of the 4 rows.
__device__ __forceinline__ const unsigned char* tb16_tr_base(const unsigned char* tile, int stride, int lane) {
    return tile + (4 * (lane >> 4) + ((lane & 15) >> 2)) * stride + 4 * (lane & 3) * 2;
}
__device__ __forceinline__ ta_bf16x8 tb16_tr_frag(const unsigned char* p0, int stride) {
    const ta_s16x4 v0 = ta_tr_read(p0), v1 = ta_tr_read(p0 + 16 * stride);
    return __builtin_bit_cast(ta_bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ------------------------------------------------------------------ dK, dV
template <int FLAGS>
__global__ __launch_bounds__(kT2Threads, 1) void k_t5_attn_bwd_dkv_d256(const TbArgs a) {
    constexpr bool BIAS = FLAGS & kTaBias, MASK = FLAGS & kTaMask, CAUSAL = FLAGS & kTaCausal;
    constexpr int KT = kTb256KvKTile, QT = kTb256KvQTile;
    constexpr int CPR = kT2D / 8;                           // 16-byte chunks per row
    constexpr int NC = QT * CPR / kT2Threads;               // chunks per thread and operand
    constexpr int LS = 2 * kT2D + 16;                       // row stride of the Q, dO and staging tiles, bytes
    constexpr int KK = kT2D / 32;                           // k-steps over d
    constexpr int DB = kT2D / 16;                           // 16-row blocks of dK^T, dV^T
    constexpr int BW = KT + QT;                             // offsets (key - query) a tile pair can meet, rounded up
    constexpr int kBytes = 2 * QT * LS;
    static_assert(KT * LS <= kBytes, "dK and dV are staged through the tiles' LDS");
    static_assert(NC * kT2Threads == QT * CPR && QT == 32 && KT == 16 * (kT2Threads / kWave) && BW <= kT2Threads, "tile geometry");
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
    __shared__ float s_bias[BW];
    __shared__ float s_lse[QT];
    __shared__ float s_delta[QT];
    unsigned char* sQ = smem;
    unsigned char* sD = smem + QT * LS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;
    int bid = blockIdx.x;
    const int kblk = bid % a.nblk;
    bid /= a.nblk;
    const int h = bid % a.nH, b = bid / a.nH;
    const int k0 = kblk * KT;
    const int kw0 = k0 + wave * 16;        // this wave's first key
    const int kg = kw0 + n;                // this lane's key

    bool live = kg < a.S;
    if (MASK) live = live && a.mask[int64_t(b) * a.S + (live ? kg : 0)] != 0;
    const bool wave_live = __ballot(live) != 0;
    const int any_live = __syncthreads_or(live ? 1 : 0);

    uint16_t* dkbase = a.dk + int64_t(b) * a.dk_sb + int64_t(h) * a.dk_sh;
    uint16_t* dvbase = a.dv + int64_t(b) * a.dv_sb + int64_t(h) * a.dv_sh;
    if (!any_live) {   // a block of dead keys: zeros, nothing read
#pragma unroll
        for (int i = 0; i < KT * CPR / kT2Threads; ++i) {
            const int cid = tid + kT2Threads * i;
            const int row = cid / CPR, ch = cid % CPR;
            if (k0 + row < a.S) {
                *reinterpret_cast<vec4u*>(dkbase + int64_t(k0 + row) * a.dk_st + ch * 8) = vec4u_make(0, 0, 0, 0);
                *reinterpret_cast<vec4u*>(dvbase + int64_t(k0 + row) * a.dv_st + ch * 8) = vec4u_make(0, 0, 0, 0);
            }
        }
        return;
    }

    // the wave's K and V fragments: lane (n, g) holds row kg, d = 32 kk + 8 g + 0..7; a dead key's are zeros
    ta_bf16x8 kf[KK], vf[KK];
    {
        const uint16_t* kp = a.k + int64_t(b) * a.k_sb + int64_t(live ? kg : 0) * a.k_st + int64_t(h) * a.k_sh + 8 * g;
        const uint16_t* vp = a.v + int64_t(b) * a.v_sb + int64_t(live ? kg : 0) * a.v_st + int64_t(h) * a.v_sh + 8 * g;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            kf[kk] = tb2_zero_frag();
            vf[kk] = tb2_zero_frag();
            if (live) {
                kf[kk] = *reinterpret_cast<const ta_bf16x8*>(kp + 32 * kk);
                vf[kk] = *reinterpret_cast<const ta_bf16x8*>(vp + 32 * kk);
            }
        }
    }
    const uint16_t* qbase = a.q + int64_t(b) * a.q_sb + int64_t(h) * a.q_sh;
    const uint16_t* gbase = a.dout + int64_t(b) * a.do_sb + int64_t(h) * a.do_sh;
    const float* lrow = a.lse + (int64_t(b) * a.nH + h) * a.Tq;
    const float* drow = a.delta + (int64_t(b) * a.nH + h) * a.Tq;
    const float* brow = BIAS ? a.bias + int64_t(h) * (a.Tq + a.S - 1) : nullptr;

    // query tiles [t_lo, t_hi): under the causal rule the queries below the block's first key see none of it
    const int t_lo = CAUSAL ? k0 / QT : 0;
    const int t_hi = (a.Tq + QT - 1) / QT;

    // tile t into registers: the rows' Q and dO chunks (zeros past Tq), lse, delta, the bias window.
    // Thread (row8 = tid >> 5, ch = tid & 31) takes chunk ch of rows row8 + 8 i.
    static_assert(CPR == 32, "a half-wave a row");
    const int prow = tid >> 5, pch = tid & 31;
    vec4u qr[NC], gr[NC];
    float br = 0.f, lr = INFINITY, der = 0.f;
    auto prefetch = [&](int t) __attribute__((always_inline)) {
        const int q0 = t * QT;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int row = prow + 8 * i;
            qr[i] = vec4u_make(0, 0, 0, 0);
            gr[i] = qr[i];
            if (q0 + row < a.Tq) {
                qr[i] = *reinterpret_cast<const vec4u*>(qbase + int64_t(q0 + row) * a.q_st + pch * 8);
                gr[i] = *reinterpret_cast<const vec4u*>(gbase + int64_t(q0 + row) * a.do_st + pch * 8);
            }
        }
        if (tid < QT) {
            const bool in = q0 + tid < a.Tq;
            lr = in ? lrow[q0 + tid] : INFINITY;
            der = in ? drow[q0 + tid] : 0.f;
        }
        if (BIAS && tid < BW) {   // entry e is the offset (key - query) = k0 - (q0 + QT - 1) + e
            const int idx = k0 - q0 - (QT - 1) + (a.Tq - 1) + tid;
            br = idx >= 0 && idx < a.Tq + a.S - 1 ? brow[idx] : 0.f;
        }
    };

    tb_f32x4 dK[DB], dV[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dK[db][i] = 0.f;
            dV[db][i] = 0.f;
        }

    if (t_lo < t_hi) prefetch(t_lo);
#pragma unroll 1
    for (int t = t_lo; t < t_hi; ++t) {
        const int q0 = t * QT;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int row = prow + 8 * i;
            *reinterpret_cast<vec4u*>(sQ + row * LS + pch * 16) = qr[i];
            *reinterpret_cast<vec4u*>(sD + row * LS + pch * 16) = gr[i];
        }
        if (tid < QT) {
            s_lse[tid] = lr;
            s_delta[tid] = der;
        }
        if (BIAS && tid < BW) s_bias[tid] = br;
        __syncthreads();
        if (t + 1 < t_hi) prefetch(t + 1);   // in flight under the MFMAs below

        if (wave_live && (!CAUSAL || q0 + QT - 1 >= kw0)) {
            // S = Q·K^T and dP = dO·V^T, two blocks of 16 queries: the key on the lane, 4 queries a block in the registers
            tb_f32x4 sacc[2], dacc[2];
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sacc[qb][i] = 0.f;
                    dacc[qb][i] = 0.f;
                }
            const unsigned char* qp = sQ + n * LS + 16 * g;
            const unsigned char* gp = sD + n * LS + 16 * g;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
                    const ta_bf16x8 qfr = *reinterpret_cast<const ta_bf16x8*>(qp + 16 * qb * LS + 64 * kk);
                    sacc[qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfr, kf[kk], sacc[qb], 0, 0, 0);
                    const ta_bf16x8 gfr = *reinterpret_cast<const ta_bf16x8*>(gp + 16 * qb * LS + 64 * kk);
                    dacc[qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gfr, vf[kk], dacc[qb], 0, 0, 0);
                }
            // P = exp(s - lse), dS = P (dP - delta); exact zeros where the key is excluded
            ta_bf16x8 pf, sf;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ql = 16 * qb + 4 * g + i;             // query in the tile
                    float s = sacc[qb][i];
                    if (BIAS) s += s_bias[(wave * 16 + n) - ql + (QT - 1)];
                    bool dead = !live || q0 + ql >= a.Tq;
                    if (CAUSAL) dead = dead || kg > q0 + ql;
                    const float p = dead ? 0.f : exp2_fast((s - s_lse[ql]) * kT2L2E);
                    const float ds = dead ? 0.f : p * (dacc[qb][i] - s_delta[ql]);
                    pf[4 * qb + i] = static_cast<__bf16>(p);
                    sf[4 * qb + i] = static_cast<__bf16>(ds);
                }
            __builtin_amdgcn_sched_barrier(0);
            // dV^T += dO^T·P, dK^T += Q^T·dS: one k = 32 step over the tile's queries per 16-row block
            const unsigned char* tg = tb16_tr_base(sD, LS, lane);
            const unsigned char* tq = tb16_tr_base(sQ, LS, lane);
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const ta_bf16x8 gt = tb16_tr_frag(tg + 32 * db, LS);
                dV[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gt, pf, dV[db], 0, 0, 0);
                const ta_bf16x8 qt = tb16_tr_frag(tq + 32 * db, LS);
                dK[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, sf, dK[db], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // round once, stage the wave's 16 rows in LDS and store whole rows: dK, then dV.  Lane (n, g) holds
    // d = 16 db + 4 g + 0..3 of key n.
    unsigned char* sO = smem + wave * 16 * LS;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const tb_f32x4& acc = which == 0 ? dK[db] : dV[db];
            uint2 pk;
            pk.x = pack_bf2(acc[0], acc[1]);
            pk.y = pack_bf2(acc[2], acc[3]);
            *reinterpret_cast<uint2*>(sO + n * LS + (16 * db + 4 * g) * 2) = pk;
        }
        __syncthreads();
        uint16_t* obase = which == 0 ? dkbase : dvbase;
        const int64_t o_st = which == 0 ? a.dk_st : a.dv_st;
#pragma unroll
        for (int i = 0; i < 16 * CPR / kWave; ++i) {
            const int cid = lane + kWave * i;
            const int row = cid / CPR, ch = cid % CPR;
            if (kw0 + row < a.S)
                *reinterpret_cast<vec4u*>(obase + int64_t(kw0 + row) * o_st + ch * 8) =
                    *reinterpret_cast<const vec4u*>(sO + row * LS + ch * 16);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dQ (and dbias)
// ORD (with DBIAS): the ordered bias gradient, as in k_t5_attn_bwd_dq.  The lane layout of the dS^T
// tile is that kernel's at one 32-key block a tile: lane (c, hh) holds query qw0 + c and, per
// register, key kl0 + 4 hh, so the 32 lanes of a half-wave meet 32 different offsets in one
// instruction, and a ring per (wave, half-wave) is summed in program order.  The window is BW = 160
// offsets and moves by 32; the hand-over sums the 8 rings in a fixed order into the workgroup's own
// partial row (a.dbias = [B, nH, nblk, S + QT - 1]) and `fill` stores the zeros of what no window
// reached: every entry of the row is stored exactly once.
template <int FLAGS, bool DBIAS, bool ORD = false>
__global__ __launch_bounds__(kT2Threads, 1) void k_t5_attn_bwd_dq_d256(const TbArgs a) {
    static_assert(DBIAS || !ORD, "the ordered form is a dbias form");
    constexpr bool BIAS = FLAGS & kTaBias, MASK = FLAGS & kTaMask, CAUSAL = FLAGS & kTaCausal;
    constexpr int QT = kTb256DqQTile, KVT = kTb256DqKVTile;
    constexpr int CPR = kT2D / 8;                           // 16-byte chunks per row
    constexpr int NC = KVT * CPR / kT2Threads;              // chunks per thread and operand
    constexpr int KS = 2 * kT2D + 16;                       // K row stride in LDS, bytes (the forward's)
    constexpr int VS = 2 * kT2D + 64;                       // V row stride (the forward's)
    constexpr int KK = kT2D / 16;                           // k-steps over d
    constexpr int DB = kT2D / 32;                           // 32-row blocks of dQ^T
    constexpr int OP = 2;                                   // passes of the staged dQ, by columns
    constexpr int OC = kT2D / OP;                           // columns per pass
    constexpr int OS = 2 * OC + 16;                         // staged dQ row stride
    constexpr int BW = QT + KVT;                            // offsets (key - query) a tile pair can meet, rounded up
    constexpr int kBytes = KVT * (KS + VS);
    static_assert(KVT == 32 && QT == 128 && NC * kT2Threads == KVT * CPR && CPR == 32, "tile geometry");
    static_assert(QT * OS <= kBytes && DB % OP == 0, "dQ is staged through the K/V tiles' LDS");
    static_assert(BW + KVT <= kT2Ring && (kT2Ring & (kT2Ring - 1)) == 0 && kT2Ring == kT2Threads && BW <= kT2Threads, "dbias ring");
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
    __shared__ float s_bias[BW];
    __shared__ float s_db[DBIAS ? (ORD ? kT2Rings : 1) * kT2Ring : 1];
    __shared__ int s_lohi[2];
    unsigned char* sK = smem;
    unsigned char* sV = smem + KVT * KS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    int bid = blockIdx.x;
    const int qb = bid % a.nblk;
    bid /= a.nblk;
    const int h = bid % a.nH, b = bid / a.nH;
    const int q0 = qb * QT;
    const int qw0 = q0 + wave * 32;        // this wave's first query
    const int qg = qw0 + c;                // this lane's query
    const int qmax = min(q0 + QT - 1, a.Tq - 1);
    const bool wave_live = qw0 < a.Tq;

    if (DBIAS) s_db[tid] = 0.f;            // kT2Ring == kT2Threads; the first tile's barrier orders it
    if (ORD) {
#pragma unroll
        for (int r = 1; r < kT2Rings; ++r) s_db[r * kT2Ring + tid] = 0.f;
    }

    // Q^T and dO^T fragments: lane (c, hh) holds row qg, d = 16 kk + 8 hh + 0..7; rows past Tq are clamped
    ta_bf16x8 qf[KK], gf[KK];
    {
        const int qc = min(qg, a.Tq - 1);
        const uint16_t* qp = a.q + int64_t(b) * a.q_sb + int64_t(qc) * a.q_st + int64_t(h) * a.q_sh + 8 * hh;
        const uint16_t* gp = a.dout + int64_t(b) * a.do_sb + int64_t(qc) * a.do_st + int64_t(h) * a.do_sh + 8 * hh;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            qf[kk] = *reinterpret_cast<const ta_bf16x8*>(qp + 16 * kk);
            gf[kk] = *reinterpret_cast<const ta_bf16x8*>(gp + 16 * kk);
        }
    }
    // a row past Tq gets lse = +inf: its P and dS are zeros
    const float lse = qg < a.Tq ? a.lse[(int64_t(b) * a.nH + h) * a.Tq + qg] : INFINITY;
    const float delta = qg < a.Tq ? a.delta[(int64_t(b) * a.nH + h) * a.Tq + qg] : 0.f;
    const uint16_t* kbase = a.k + int64_t(b) * a.k_sb + int64_t(h) * a.k_sh;
    const uint16_t* vbase = a.v + int64_t(b) * a.v_sb + int64_t(h) * a.v_sh;
    const float* brow = BIAS ? a.bias + int64_t(h) * (a.Tq + a.S - 1) : nullptr;
    const int prl = a.S + QT - 1;          // ORD: entries of a partial row
    float* dbrow = !DBIAS ? nullptr
                   : ORD  ? a.dbias + ((int64_t(b) * a.nH + h) * a.nblk + qb) * prl
                          : a.dbias + int64_t(h) * (a.Tq + a.S - 1);
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
        for (int j = tid; j < kend; j += kT2Threads)
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
    // wave's 64 lanes take two whole 512-byte rows per chunk index (row 2 wave + 8 i + hh of the tile).
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
        for (int i = 0; i < NC; ++i) {
            const int ur = 2 * wave + 8 * i;
            kr[i] = vec4u_make(0, 0, 0, 0);
            vr[i] = kr[i];
            if ((lmN >> (ur + hh)) & 1) {
                kr[i] = *reinterpret_cast<const vec4u*>(klane + int64_t(k0 + ur) * a.k_st);
                vr[i] = *reinterpret_cast<const vec4u*>(vlane + int64_t(k0 + ur) * a.v_st);
            }
        }
        if (BIAS && tid < BW) {   // entry e is the offset (key - query) = k0 - (q0 + 127) + e
            const int idx = k0 - q0 - (QT - 1) + (a.Tq - 1) + tid;
            br = idx >= 0 && idx < a.Tq + a.S - 1 ? brow[idx] : 0.f;
        }
    };
    // dbias: ring slot of table index idx (ORD: of the row's local index), and the hand-over of one
    // index to the global buffer
    int ring0 = 0;              // table (ORD: local) index of the current tile's window entry 0
    bool ring_open = false;
    auto flush = [&](int idx) __attribute__((always_inline)) {
        float* slot = &s_db[idx & (kT2Ring - 1)];
        if (ORD) {
            float x = 0.f;
#pragma unroll 1   // rolled: eight reads in flight here spill the bias form without a mask (512 registers in use)
            for (int r = 0; r < kT2Rings; ++r) {
                x += slot[r * kT2Ring];
                slot[r * kT2Ring] = 0.f;
            }
            if (idx < prl) dbrow[idx] = x;   // idx >= 0: a window starts at its tile's first key
            return;
        }
        const float x = *slot;
        *slot = 0.f;
        if (!(x == 0.f) && idx >= 0 && idx < a.Tq + a.S - 1) atomicAdd(dbrow + idx, x);
    };
    auto fill = [&](int from, int upto) __attribute__((always_inline)) {   // ORD: zeros for [from, upto)
        for (int j = from + tid; j < upto; j += kT2Threads) dbrow[j] = 0.f;
    };
    const int ring = (2 * wave + hh) * kT2Ring;   // ORD: this half-wave's ring

    ta_f32x16 dQ[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) dQ[db][i] = 0.f;

    if (t_lo < t_hi) prefetch(t_lo);
    if (ORD) fill(0, t_lo < t_hi ? t_lo * KVT : 0);   // below the first window: zeros
#pragma unroll 1
    for (int t = t_lo; t < t_hi; ++t) {
        const unsigned long long lm = lmN;
        const int k0 = t * KVT;
        if (lm) {
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const int row = 2 * wave + 8 * i + hh;
                *reinterpret_cast<vec4u*>(sK + row * KS + c * 16) = kr[i];
                *reinterpret_cast<vec4u*>(sV + row * VS + c * 16) = vr[i];
            }
            if (BIAS && tid < BW) s_bias[tid] = br;
            if (DBIAS && !ORD) {   // the offsets below the new window are complete: hand them over
                const int nb = k0 - q0 - (QT - 1) + (a.Tq - 1);
                if (ring_open && tid < BW && ring0 + tid < nb) flush(ring0 + tid);
                ring0 = nb;
                ring_open = true;
            }
        }
        if (ORD) {   // at every tile, a dead one too: the windows follow each other and leave no gap in the row
            if (ring_open && tid < KVT) flush(ring0 + tid);
            ring0 = k0;
            ring_open = true;
        }
        __syncthreads();
        if (t + 1 < t_hi) prefetch(t + 1);   // in flight under the MFMAs below

        const bool active = lm != 0 && wave_live && (!CAUSAL || k0 <= min(qw0 + 31, a.Tq - 1));
        if (active) {
            // S^T = K·Q^T and dP^T = V·dO^T for the tile's 32 keys: the query on the lane
            ta_f32x16 sacc, dacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                sacc[i] = 0.f;
                dacc[i] = 0.f;
            }
            const unsigned char* kp = sK + c * KS + 16 * hh;
            const unsigned char* vp = sV + c * VS + 16 * hh;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const ta_bf16x8 kfr = *reinterpret_cast<const ta_bf16x8*>(kp + 32 * kk);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr, qf[kk], sacc, 0, 0, 0);
                const ta_bf16x8 vfr = *reinterpret_cast<const ta_bf16x8*>(vp + 32 * kk);
                dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr, gf[kk], dacc, 0, 0, 0);
                if ((kk & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four k-steps' row fragments live at a time
            }
            // P = exp(s - lse), dS = P (dP - delta); exact zeros where the key is excluded
            const uint32_t w = uint32_t(lm) >> (4 * hh);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kl0 = (i & 3) + 8 * (i >> 2);        // key in the tile, less 4 hh
                const int kl = kl0 + 4 * hh;
                const int e = kl - (wave * 32 + c) + (QT - 1);
                float s = sacc[i];
                if (BIAS) s += s_bias[e];
                bool dead = !((w >> kl0) & 1u) || qg >= a.Tq;
                if (CAUSAL) dead = dead || k0 + kl > qg;
                const float p = dead ? 0.f : exp2_fast((s - lse) * kT2L2E);
                const float ds = dead ? 0.f : p * (dacc[i] - delta);
                if (DBIAS) atomicAdd(&s_db[(ORD ? ring : 0) + ((ring0 + e) & (kT2Ring - 1))], ds);   // a dead pair adds its exact zero: no branch
                sacc[i] = ds;
            }
            __builtin_amdgcn_sched_barrier(0);
            // dQ^T += K^T·dS^T
            const unsigned char* tk = ta_tr_base(sK, KS, lane);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                ta_bf16x8 sf;
#pragma unroll
                for (int j = 0; j < 8; ++j) sf[j] = static_cast<__bf16>(sacc[8 * s2 + j]);
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const ta_bf16x8 kt = ta_tr_frag(tk + 16 * s2 * KS + 64 * db, KS);
                    dQ[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt, sf, dQ[db], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);   // one k-step's K^T fragments live at a time
            }
        }
        __syncthreads();
    }
    if (DBIAS) {
        if (ring_open && tid < BW) flush(ring0 + tid);
        if (ORD) fill(ring_open ? ring0 + BW : 0, prl);   // past the last window, or a walk of no tile: zeros
    }

    // round once, stage the wave's 32 rows in LDS (OC columns a pass) and store whole rows
    unsigned char* sO = smem + wave * 32 * OS;
    uint16_t* obase = a.dq + int64_t(b) * a.dq_sb + int64_t(h) * a.dq_sh;
#pragma unroll
    for (int p = 0; p < OP; ++p) {
        if (p) __syncthreads();
#pragma unroll
        for (int dbl = 0; dbl < DB / OP; ++dbl)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const ta_f32x16& acc = dQ[p * (DB / OP) + dbl];
                uint2 pk;
                pk.x = pack_bf2(acc[4 * gq], acc[4 * gq + 1]);
                pk.y = pack_bf2(acc[4 * gq + 2], acc[4 * gq + 3]);
                *reinterpret_cast<uint2*>(sO + c * OS + (32 * dbl + 8 * gq + 4 * hh) * 2) = pk;
            }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 32 * (OC / 8) / kWave; ++i) {
            const int cid = lane + kWave * i;
            const int row = cid / (OC / 8), ch = cid % (OC / 8);
            if (qw0 + row < a.Tq)
                *reinterpret_cast<vec4u*>(obase + int64_t(qw0 + row) * a.dq_st + p * OC + ch * 8) =
                    *reinterpret_cast<const vec4u*>(sO + row * OS + ch * 16);
        }
    }
}

typedef void (*tb2_kernel_t)(const TbArgs);
static tb2_kernel_t tb2_pick_dkv(int flags) {
    switch (flags) {
        case 0: return k_t5_attn_bwd_dkv_d256<0>;
        case 1: return k_t5_attn_bwd_dkv_d256<1>;
        case 2: return k_t5_attn_bwd_dkv_d256<2>;
        case 3: return k_t5_attn_bwd_dkv_d256<3>;
        case 4: return k_t5_attn_bwd_dkv_d256<4>;
        case 5: return k_t5_attn_bwd_dkv_d256<5>;
        case 6: return k_t5_attn_bwd_dkv_d256<6>;
        default: return k_t5_attn_bwd_dkv_d256<7>;
    }
}
template <bool DBIAS, bool ORD = false>
static tb2_kernel_t tb2_pick_dq(int flags) {
    switch (flags) {
        case 0: return k_t5_attn_bwd_dq_d256<0, DBIAS, ORD>;
        case 1: return k_t5_attn_bwd_dq_d256<1, DBIAS, ORD>;
        case 2: return k_t5_attn_bwd_dq_d256<2, DBIAS, ORD>;
        case 3: return k_t5_attn_bwd_dq_d256<3, DBIAS, ORD>;
        case 4: return k_t5_attn_bwd_dq_d256<4, DBIAS, ORD>;
        case 5: return k_t5_attn_bwd_dq_d256<5, DBIAS, ORD>;
        case 6: return k_t5_attn_bwd_dq_d256<6, DBIAS, ORD>;
        default: return k_t5_attn_bwd_dq_d256<7, DBIAS, ORD>;
    }
}

int tb_launch_d256(TbArgs k, int flags, unsigned grid_k, unsigned grid_q, bool ordered, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    k.nblk = (k.S + kTb256KvKTile - 1) / kTb256KvKTile;
    hipLaunchKernelGGL(tb2_pick_dkv(flags), dim3(grid_k), dim3(kT2Threads), 0, st, k);
    const int rc = check_launch("k_t5_attn_bwd_dkv_d256");
    if (rc != TRLX_OK) return rc;
    k.nblk = (k.Tq + kTb256DqQTile - 1) / kTb256DqQTile;
    const tb2_kernel_t fn = !k.dbias ? tb2_pick_dq<false>(flags) : ordered ? tb2_pick_dq<true, true>(flags) : tb2_pick_dq<true>(flags);
    hipLaunchKernelGGL(fn, dim3(grid_q), dim3(kT2Threads), 0, st, k);
    return check_launch("k_t5_attn_bwd_dq_d256");
}

}  // namespace trlx
