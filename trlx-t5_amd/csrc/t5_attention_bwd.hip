// T5 full-sequence attention backward: dq, dk, dv and the gradient of the relative-position bias
// table, with nothing of size Tq x S held.  See trlx_t5_attention_bwd in trlx_t5_amd.h; the forward
// is t5_attention.hip, whose row statistics lse = m + log(l) (trlx_t5_attention_fwd_lse) let every
// tile rebuild P = exp(s - lse) on its own.
//
// Three launches, all on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
//   k_t5_attn_bwd_delta   delta[b, h, i] = sum_d dO_i · O_i, fp32, one wave per 32 rows (the diagonal of
//                         dO·O^T, so that it is summed exactly as dP is).
//   k_t5_attn_bwd_dkv     one workgroup = 4 waves = one (batch row, head, block of kTbKvKTile = 128
//                         keys); a wave owns 32 keys, keeps their K and V fragments and dK^T, dV^T in
//                         registers and walks the queries in LDS tiles of kTbKvQTile = 64 rows of Q
//                         and dO (global -> registers one tile ahead -> LDS).
//   k_t5_attn_bwd_dq      one workgroup = one (batch row, head, block of kTbDqQTile = 128 queries),
//                         the forward's own walk: a wave owns 32 queries, keeps their Q^T and dO^T
//                         fragments and dQ^T in registers and walks the keys in LDS tiles of
//                         kTbDqKVTile = 64 rows of K and V.  With DBIAS it also sums dS by offset.
// S is recomputed in both: the price of dq, dk and dv without a global atomic, each summed in an
// order fixed by (d_kv, Tq, S, the flags, the mask row).
//
// Orientation.  dkv: S = Q·K^T (A = Q rows from LDS, B = the wave's K fragments), so a 32x32 result
// has its KEY on the lane and 16 of the 32 queries in the registers; lse and delta are read per
// register from LDS.  P and dS = P (dP - delta), rounded to bf16, are directly the B operands of
// dV^T = dO^T·P and dK^T = Q^T·dS, whose A operands come out of the row-major dO and Q tiles through
// the transposed LDS read (ta_tr_frag).  dq: S^T = K·Q^T as in the forward, the QUERY on the lane,
// lse and delta one value per lane; dS^T is the B operand of dQ^T = K^T·dS^T.
//
// Keys and rows.  A dead key (out of range, key_mask == 0) is never read: its fragments / LDS rows
// are zeros and its P and dS are selected to exact zeros, so its dK and dV rows are zeros.  A block
// of keys with no live key writes zeros and leaves; tiles with no live key and tiles above the
// causal diagonal are skipped.  Query rows past Tq are zeros in LDS with lse = +inf.  A query
// without a live key has lse = +inf, so P = 0 and its dQ row is zeros.
//
// dbias.  Each dq workgroup adds its dS into an LDS ring of kTbRing offsets (LDS fp32 atomics); the
// 64 offsets that leave the window when the walk moves on one tile are flushed to the
// [nH, Tq + S - 1] buffer with global fp32 atomics.  Not bit-reproducible.
#include <climits>

#include "t5_attention.h"

namespace trlx {

constexpr int kTbThreads = 256;
constexpr int kTbDqQTile = 128;   // dq: query rows per workgroup (32 per wave)
constexpr int kTbDqKVTile = 64;   // dq: keys per LDS tile
constexpr int kTbKvKTile = 128;   // dkv: keys per workgroup (32 per wave)
constexpr int kTbKvQTile = 64;    // dkv: query rows per LDS tile
constexpr int kTbWin = 192;       // offsets (key - query) a 128 x 64 tile pair can meet, rounded up
constexpr int kTbRing = 256;      // dbias ring in LDS (a power of two >= kTbWin)
constexpr float kTbL2E = 1.4426950408889634f;

struct TbArgs {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    const uint16_t* o;
    const uint16_t* dout;
    uint16_t* dq;
    uint16_t* dk;
    uint16_t* dv;
    const float* lse;      // [B, nH, Tq]
    float* delta;          // [B, nH, Tq]
    const float* bias;     // [nH, Tq + S - 1] or NULL
    const int64_t* mask;   // [B, S] or NULL
    float* dbias;          // [nH, Tq + S - 1] or NULL
    int64_t q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh, do_sb, do_st, do_sh;
    int64_t dq_sb, dq_st, dq_sh, dk_sb, dk_st, dk_sh, dv_sb, dv_st, dv_sh;
    int nH, Tq, S, nblk;
};

__device__ __forceinline__ ta_bf16x8 tb_zero_frag() { return __builtin_bit_cast(ta_bf16x8, vec4u_make(0, 0, 0, 0)); }

// ------------------------------------------------------------------ delta = rowsum(dO * O)
// One wave per 32 rows, as the diagonal of dO·O^T through the same MFMA chain over d that dP = dO·V^T
// takes in the other two kernels: where a query has ONE live key its O row is that key's V row bit
// for bit, delta equals dP bit for bit, and dS = P (dP - delta) is the exact zero it is in
// arithmetic (a fp32 row sum in another order leaves ~1e-6 there, where torch's softmax backward
// gives 0).  Lane (c, hh) finds row c's diagonal element in register (c & 3) + 4 (c >> 3) if
// hh == (c >> 2) & 1.
template <int DKV>
__global__ __launch_bounds__(kTbThreads) void k_t5_attn_bwd_delta(const TbArgs a, const int nrb, const int64_t nwaves) {
    constexpr int KK = DKV / 16;
    const int lane = threadIdx.x & 63;
    const int c = lane & 31, hh = lane >> 5;
    const int64_t wid = int64_t(blockIdx.x) * (kTbThreads / kWave) + (threadIdx.x >> 6);
    if (wid >= nwaves) return;
    const int rb = int(wid % nrb);
    const int64_t bh = wid / nrb;
    const int h = int(bh % a.nH);
    const int64_t b = bh / a.nH;
    const int row = rb * 32 + c;
    const int rc = min(row, a.Tq - 1);   // rows past Tq are clamped and not stored
    const uint16_t* gp = a.dout + b * a.do_sb + int64_t(rc) * a.do_st + int64_t(h) * a.do_sh + 8 * hh;
    const uint16_t* op = a.o + b * a.o_sb + int64_t(rc) * a.o_st + int64_t(h) * a.o_sh + 8 * hh;
    ta_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        const ta_bf16x8 gfr = *reinterpret_cast<const ta_bf16x8*>(gp + 16 * kk);
        const ta_bf16x8 ofr = *reinterpret_cast<const ta_bf16x8*>(op + 16 * kk);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gfr, ofr, acc, 0, 0, 0);
    }
    const int want = (c & 3) + 4 * (c >> 3);
    float dl = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) dl = i == want ? acc[i] : dl;
    if (hh == ((c >> 2) & 1) && row < a.Tq) a.delta[bh * a.Tq + row] = dl;
}

// ------------------------------------------------------------------ dK, dV
template <int DKV, int FLAGS>
__global__ __launch_bounds__(kTbThreads, DKV == 64 ? 2 : 1) void k_t5_attn_bwd_dkv(const TbArgs a) {
    constexpr bool BIAS = FLAGS & kTaBias, MASK = FLAGS & kTaMask, CAUSAL = FLAGS & kTaCausal;
    constexpr int CPR = DKV / 8;                            // 16-byte chunks per row
    constexpr int NC = kTbKvQTile * CPR / kTbThreads;       // chunks per thread and operand
    constexpr int LS = 2 * DKV + 16;                        // row stride of the Q, dO and staging tiles, bytes
    constexpr int KK = DKV / 16;                            // k-steps over d
    constexpr int DB = DKV / 32;                            // 32-row blocks of dK^T, dV^T
    constexpr int kBytes = 2 * kTbKvQTile * LS;
    static_assert(kTbKvKTile * LS <= kBytes, "dK and dV are staged through the tiles' LDS");
    static_assert(NC * kTbThreads == kTbKvQTile * CPR && kTbKvQTile == 64 && kTbKvKTile == 128, "tile geometry");
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
    __shared__ float s_bias[kTbWin];
    __shared__ float s_lse[kTbKvQTile];
    __shared__ float s_delta[kTbKvQTile];
    unsigned char* sQ = smem;
    unsigned char* sD = smem + kTbKvQTile * LS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    int bid = blockIdx.x;
    const int kblk = bid % a.nblk;
    bid /= a.nblk;
    const int h = bid % a.nH, b = bid / a.nH;
    const int k0 = kblk * kTbKvKTile;
    const int kw0 = k0 + wave * 32;        // this wave's first key
    const int kg = kw0 + c;                // this lane's key

    bool live = kg < a.S;
    if (MASK) live = live && a.mask[int64_t(b) * a.S + (live ? kg : 0)] != 0;
    const bool wave_live = __ballot(live) != 0;
    const int any_live = __syncthreads_or(live ? 1 : 0);

    uint16_t* dkbase = a.dk + int64_t(b) * a.dk_sb + int64_t(h) * a.dk_sh;
    uint16_t* dvbase = a.dv + int64_t(b) * a.dv_sb + int64_t(h) * a.dv_sh;
    if (!any_live) {   // a block of dead keys: zeros, nothing read
#pragma unroll
        for (int n = 0; n < kTbKvKTile * CPR / kTbThreads; ++n) {
            const int cid = tid + kTbThreads * n;
            const int row = cid / CPR, ch = cid % CPR;
            if (k0 + row < a.S) {
                *reinterpret_cast<vec4u*>(dkbase + int64_t(k0 + row) * a.dk_st + ch * 8) = vec4u_make(0, 0, 0, 0);
                *reinterpret_cast<vec4u*>(dvbase + int64_t(k0 + row) * a.dv_st + ch * 8) = vec4u_make(0, 0, 0, 0);
            }
        }
        return;
    }

    // the wave's K and V fragments: lane (c, hh) holds row kg, d = 16 kk + 8 hh + 0..7; a dead key's are zeros
    ta_bf16x8 kf[KK], vf[KK];
    {
        const uint16_t* kp = a.k + int64_t(b) * a.k_sb + int64_t(live ? kg : 0) * a.k_st + int64_t(h) * a.k_sh + 8 * hh;
        const uint16_t* vp = a.v + int64_t(b) * a.v_sb + int64_t(live ? kg : 0) * a.v_st + int64_t(h) * a.v_sh + 8 * hh;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            kf[kk] = tb_zero_frag();
            vf[kk] = tb_zero_frag();
            if (live) {
                kf[kk] = *reinterpret_cast<const ta_bf16x8*>(kp + 16 * kk);
                vf[kk] = *reinterpret_cast<const ta_bf16x8*>(vp + 16 * kk);
            }
        }
    }
    const uint16_t* qbase = a.q + int64_t(b) * a.q_sb + int64_t(h) * a.q_sh;
    const uint16_t* gbase = a.dout + int64_t(b) * a.do_sb + int64_t(h) * a.do_sh;
    const float* lrow = a.lse + (int64_t(b) * a.nH + h) * a.Tq;
    const float* drow = a.delta + (int64_t(b) * a.nH + h) * a.Tq;
    const float* brow = BIAS ? a.bias + int64_t(h) * (a.Tq + a.S - 1) : nullptr;

    // query tiles [t_lo, t_hi): under the causal rule the queries below the block's first key see none of it
    const int t_lo = CAUSAL ? k0 / kTbKvQTile : 0;
    const int t_hi = (a.Tq + kTbKvQTile - 1) / kTbKvQTile;

    // tile t into registers: the rows' Q and dO chunks (zeros past Tq), lse, delta, the bias window
    vec4u qr[NC], gr[NC];
    float br = 0.f, lr = INFINITY, der = 0.f;
    auto prefetch = [&](int t) __attribute__((always_inline)) {
        const int q0 = t * kTbKvQTile;
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const int cid = tid + kTbThreads * n;
            const int row = cid / CPR, ch = cid % CPR;
            qr[n] = vec4u_make(0, 0, 0, 0);
            gr[n] = qr[n];
            if (q0 + row < a.Tq) {
                qr[n] = *reinterpret_cast<const vec4u*>(qbase + int64_t(q0 + row) * a.q_st + ch * 8);
                gr[n] = *reinterpret_cast<const vec4u*>(gbase + int64_t(q0 + row) * a.do_st + ch * 8);
            }
        }
        if (tid < kTbKvQTile) {
            const bool in = q0 + tid < a.Tq;
            lr = in ? lrow[q0 + tid] : INFINITY;
            der = in ? drow[q0 + tid] : 0.f;
        }
        if (BIAS && tid < kTbWin) {   // entry e is the offset (key - query) = k0 - (q0 + 63) + e
            const int idx = k0 - q0 - (kTbKvQTile - 1) + (a.Tq - 1) + tid;
            br = idx >= 0 && idx < a.Tq + a.S - 1 ? brow[idx] : 0.f;
        }
    };

    ta_f32x16 dK[DB], dV[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            dK[db][i] = 0.f;
            dV[db][i] = 0.f;
        }

    if (t_lo < t_hi) prefetch(t_lo);
#pragma unroll 1
    for (int t = t_lo; t < t_hi; ++t) {
        const int q0 = t * kTbKvQTile;
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const int cid = tid + kTbThreads * n;
            const int row = cid / CPR, ch = cid % CPR;
            *reinterpret_cast<vec4u*>(sQ + row * LS + ch * 16) = qr[n];
            *reinterpret_cast<vec4u*>(sD + row * LS + ch * 16) = gr[n];
        }
        if (tid < kTbKvQTile) {
            s_lse[tid] = lr;
            s_delta[tid] = der;
        }
        if (BIAS && tid < kTbWin) s_bias[tid] = br;
        __syncthreads();
        if (t + 1 < t_hi) prefetch(t + 1);

        if (wave_live) {
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                const int qb0 = q0 + 32 * qb;                    // the 32-query block's first row
                if (qb0 >= a.Tq || (CAUSAL && qb0 + 31 < kw0)) continue;
                // S = Q·K^T and dP = dO·V^T: the key on the lane, 16 of the 32 queries in the registers
                ta_f32x16 sacc, dacc;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sacc[i] = 0.f;
                    dacc[i] = 0.f;
                }
                const unsigned char* qp = sQ + (32 * qb + c) * LS + 16 * hh;
                const unsigned char* gp = sD + (32 * qb + c) * LS + 16 * hh;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const ta_bf16x8 qfr = *reinterpret_cast<const ta_bf16x8*>(qp + 32 * kk);
                    sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr, kf[kk], sacc, 0, 0, 0);
                    const ta_bf16x8 gfr = *reinterpret_cast<const ta_bf16x8*>(gp + 32 * kk);
                    dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gfr, vf[kk], dacc, 0, 0, 0);
                }
                // P = exp(s - lse), dS = P (dP - delta); exact zeros where the key is excluded
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int ql = 32 * qb + (i & 3) + 8 * (i >> 2) + 4 * hh;   // query in the tile
                    float s = sacc[i];
                    if (BIAS) s += s_bias[(wave * 32 + c) - ql + (kTbKvQTile - 1)];
                    bool dead = !live || q0 + ql >= a.Tq;
                    if (CAUSAL) dead = dead || kg > q0 + ql;
                    const float p = dead ? 0.f : exp2_fast((s - s_lse[ql]) * kTbL2E);
                    const float ds = dead ? 0.f : p * (dacc[i] - s_delta[ql]);
                    sacc[i] = p;
                    dacc[i] = ds;
                }
                // dV^T += dO^T·P, dK^T += Q^T·dS
                const unsigned char* tg = ta_tr_base(sD, LS, lane) + 32 * qb * LS;
                const unsigned char* tq = ta_tr_base(sQ, LS, lane) + 32 * qb * LS;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    ta_bf16x8 pf, sf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        pf[j] = static_cast<__bf16>(sacc[8 * s2 + j]);
                        sf[j] = static_cast<__bf16>(dacc[8 * s2 + j]);
                    }
#pragma unroll
                    for (int db = 0; db < DB; ++db) {
                        const ta_bf16x8 gt = ta_tr_frag(tg + 16 * s2 * LS + 64 * db, LS);
                        dV[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gt, pf, dV[db], 0, 0, 0);
                        const ta_bf16x8 qt = ta_tr_frag(tq + 16 * s2 * LS + 64 * db, LS);
                        dK[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt, sf, dK[db], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }

    // round once, stage the wave's 32 rows in LDS and store whole rows: dK, then dV
    unsigned char* sO = smem + wave * 32 * LS;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const ta_f32x16& acc = which == 0 ? dK[db] : dV[db];
                uint2 pk;
                pk.x = pack_bf2(acc[4 * g], acc[4 * g + 1]);
                pk.y = pack_bf2(acc[4 * g + 2], acc[4 * g + 3]);
                *reinterpret_cast<uint2*>(sO + c * LS + (32 * db + 8 * g + 4 * hh) * 2) = pk;
            }
        __syncthreads();
        uint16_t* obase = which == 0 ? dkbase : dvbase;
        const int64_t o_st = which == 0 ? a.dk_st : a.dv_st;
#pragma unroll
        for (int n = 0; n < 32 * CPR / kWave; ++n) {
            const int cid = lane + kWave * n;
            const int row = cid / CPR, ch = cid % CPR;
            if (kw0 + row < a.S)
                *reinterpret_cast<vec4u*>(obase + int64_t(kw0 + row) * o_st + ch * 8) =
                    *reinterpret_cast<const vec4u*>(sO + row * LS + ch * 16);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dQ (and dbias)
template <int DKV, int FLAGS, bool DBIAS>
__global__ __launch_bounds__(kTbThreads, DKV == 64 ? 2 : 1) void k_t5_attn_bwd_dq(const TbArgs a) {
    constexpr bool BIAS = FLAGS & kTaBias, MASK = FLAGS & kTaMask, CAUSAL = FLAGS & kTaCausal;
    constexpr int CPR = DKV / 8;                            // 16-byte chunks per row
    constexpr int NC = kTbDqKVTile * CPR / kTbThreads;      // chunks per thread and operand
    constexpr int LS = 2 * DKV + 16;                        // row stride of the K, V and staging tiles, bytes
    constexpr int KK = DKV / 16;                            // k-steps over d
    constexpr int DB = DKV / 32;                            // 32-row blocks of dQ^T
    constexpr int kBytes = 2 * kTbDqKVTile * LS;
    static_assert(kTbDqQTile * LS <= kBytes, "dQ is staged through the K/V tiles' LDS");
    static_assert(NC * kTbThreads == kTbDqKVTile * CPR && kTbDqKVTile == 64 && kTbDqQTile == 128, "tile geometry");
    static_assert(kTbDqQTile + kTbDqKVTile <= kTbWin && kTbWin + kTbDqKVTile <= kTbRing && (kTbRing & (kTbRing - 1)) == 0,
                  "dbias ring");
    __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
    __shared__ float s_bias[kTbWin];
    __shared__ float s_db[DBIAS ? kTbRing : 1];
    __shared__ int s_lohi[2];
    unsigned char* sK = smem;
    unsigned char* sV = smem + kTbDqKVTile * LS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    int bid = blockIdx.x;
    const int qb = bid % a.nblk;
    bid /= a.nblk;
    const int h = bid % a.nH, b = bid / a.nH;
    const int q0 = qb * kTbDqQTile;
    const int qw0 = q0 + wave * 32;        // this wave's first query
    const int qg = qw0 + c;                // this lane's query
    const int qmax = min(q0 + kTbDqQTile - 1, a.Tq - 1);
    const bool wave_live = qw0 < a.Tq;

    if (DBIAS) s_db[tid] = 0.f;            // kTbRing == kTbThreads; the first tile's barrier orders it

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
    float* dbrow = DBIAS ? a.dbias + int64_t(h) * (a.Tq + a.S - 1) : nullptr;
    const int64_t* mrow = MASK ? a.mask + int64_t(b) * a.S : nullptr;

    // keys [0, kend) can matter to this workgroup; the tiles walked are [t_lo, t_hi)
    const int kend = CAUSAL ? min(a.S, qmax + 1) : a.S;
    int t_lo = 0, t_hi = (kend + kTbDqKVTile - 1) / kTbDqKVTile;
    if (MASK) {
        if (tid == 0) {
            s_lohi[0] = INT_MAX;
            s_lohi[1] = -1;
        }
        __syncthreads();
        int lo = INT_MAX, hi = -1;
        for (int j = tid; j < kend; j += kTbThreads)
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
        t_lo = hi < 0 ? 0 : lo / kTbDqKVTile;
        t_hi = hi < 0 ? 0 : hi / kTbDqKVTile + 1;
    }

    // tile t into registers: the live-key mask, the live rows' K and V chunks, the bias window
    vec4u kr[NC], vr[NC];
    float br = 0.f;
    unsigned long long lmN = 0;
    auto prefetch = [&](int t) __attribute__((always_inline)) {
        const int k0 = t * kTbDqKVTile;
        const int key = k0 + lane;
        bool live = key < kend;
        if (MASK) live = live && mrow[live ? key : 0] != 0;
        lmN = __ballot(live);
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const int cid = tid + kTbThreads * n;
            const int row = cid / CPR, ch = cid % CPR;
            kr[n] = vec4u_make(0, 0, 0, 0);
            vr[n] = kr[n];
            if ((lmN >> row) & 1) {
                kr[n] = *reinterpret_cast<const vec4u*>(kbase + int64_t(k0 + row) * a.k_st + ch * 8);
                vr[n] = *reinterpret_cast<const vec4u*>(vbase + int64_t(k0 + row) * a.v_st + ch * 8);
            }
        }
        if (BIAS && tid < kTbWin) {   // entry e is the offset (key - query) = k0 - (q0 + 127) + e
            const int idx = k0 - q0 - (kTbDqQTile - 1) + (a.Tq - 1) + tid;
            br = idx >= 0 && idx < a.Tq + a.S - 1 ? brow[idx] : 0.f;
        }
    };
    // dbias: ring slot of table index idx, and the hand-over of one index to the global buffer
    int ring0 = 0;              // table index of the current tile's window entry 0
    bool ring_open = false;
    auto flush = [&](int idx) __attribute__((always_inline)) {
        float* slot = &s_db[idx & (kTbRing - 1)];
        const float x = *slot;
        *slot = 0.f;
        if (!(x == 0.f) && idx >= 0 && idx < a.Tq + a.S - 1) atomicAdd(dbrow + idx, x);
    };

    ta_f32x16 dQ[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) dQ[db][i] = 0.f;

    if (t_lo < t_hi) prefetch(t_lo);
#pragma unroll 1
    for (int t = t_lo; t < t_hi; ++t) {
        const unsigned long long lm = lmN;
        const int k0 = t * kTbDqKVTile;
        if (lm) {
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int cid = tid + kTbThreads * n;
                const int row = cid / CPR, ch = cid % CPR;
                *reinterpret_cast<vec4u*>(sK + row * LS + ch * 16) = kr[n];
                *reinterpret_cast<vec4u*>(sV + row * LS + ch * 16) = vr[n];
            }
            if (BIAS && tid < kTbWin) s_bias[tid] = br;
            if (DBIAS) {   // the offsets below the new window are complete: hand them over
                const int nb = k0 - q0 - (kTbDqQTile - 1) + (a.Tq - 1);
                if (ring_open && tid < kTbWin && ring0 + tid < nb) flush(ring0 + tid);
                ring0 = nb;
                ring_open = true;
            }
        }
        __syncthreads();
        if (t + 1 < t_hi) prefetch(t + 1);

        const bool active = lm != 0 && wave_live && (!CAUSAL || k0 <= min(qw0 + 31, a.Tq - 1));
        if (active) {
            // S^T = K·Q^T and dP^T = V·dO^T, two blocks of 32 keys: the query on the lane
            ta_f32x16 sacc[2], dacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sacc[kb][i] = 0.f;
                    dacc[kb][i] = 0.f;
                }
                const unsigned char* kp = sK + (32 * kb + c) * LS + 16 * hh;
                const unsigned char* vp = sV + (32 * kb + c) * LS + 16 * hh;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const ta_bf16x8 kfr = *reinterpret_cast<const ta_bf16x8*>(kp + 32 * kk);
                    sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr, qf[kk], sacc[kb], 0, 0, 0);
                    const ta_bf16x8 vfr = *reinterpret_cast<const ta_bf16x8*>(vp + 32 * kk);
                    dacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr, gf[kk], dacc[kb], 0, 0, 0);
                }
            }
            // P = exp(s - lse), dS = P (dP - delta); exact zeros where the key is excluded
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const uint32_t w = uint32_t(lm >> (32 * kb)) >> (4 * hh);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int kl0 = (i & 3) + 8 * (i >> 2);        // key in the block, less 4 hh
                    const int kl = 32 * kb + kl0 + 4 * hh;         // key in the tile
                    const int e = kl - (wave * 32 + c) + (kTbDqQTile - 1);
                    float s = sacc[kb][i];
                    if (BIAS) s += s_bias[e];
                    bool dead = !((w >> kl0) & 1u) || qg >= a.Tq;
                    if (CAUSAL) dead = dead || k0 + kl > qg;
                    const float p = dead ? 0.f : exp2_fast((s - lse) * kTbL2E);
                    const float ds = dead ? 0.f : p * (dacc[kb][i] - delta);
                    if (DBIAS) {
                        if (!dead) atomicAdd(&s_db[(ring0 + e) & (kTbRing - 1)], ds);
                    }
                    sacc[kb][i] = ds;
                }
            }
            // dQ^T += K^T·dS^T
            const unsigned char* tk = ta_tr_base(sK, LS, lane);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    ta_bf16x8 sf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) sf[j] = static_cast<__bf16>(sacc[kb][8 * s2 + j]);
#pragma unroll
                    for (int db = 0; db < DB; ++db) {
                        const ta_bf16x8 kt = ta_tr_frag(tk + (32 * kb + 16 * s2) * LS + 64 * db, LS);
                        dQ[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt, sf, dQ[db], 0, 0, 0);
                    }
                }
        }
        __syncthreads();
    }
    if (DBIAS) {
        if (ring_open && tid < kTbWin) flush(ring0 + tid);
    }

    // round once, stage the wave's 32 rows in LDS and store whole rows
    unsigned char* sO = smem + wave * 32 * LS;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 pk;
            pk.x = pack_bf2(dQ[db][4 * g], dQ[db][4 * g + 1]);
            pk.y = pack_bf2(dQ[db][4 * g + 2], dQ[db][4 * g + 3]);
            *reinterpret_cast<uint2*>(sO + c * LS + (32 * db + 8 * g + 4 * hh) * 2) = pk;
        }
    __syncthreads();
    uint16_t* obase = a.dq + int64_t(b) * a.dq_sb + int64_t(h) * a.dq_sh;
#pragma unroll
    for (int n = 0; n < 32 * CPR / kWave; ++n) {
        const int cid = lane + kWave * n;
        const int row = cid / CPR, ch = cid % CPR;
        if (qw0 + row < a.Tq)
            *reinterpret_cast<vec4u*>(obase + int64_t(qw0 + row) * a.dq_st + ch * 8) =
                *reinterpret_cast<const vec4u*>(sO + row * LS + ch * 16);
    }
}

typedef void (*tb_kernel_t)(const TbArgs);
template <int DKV>
static tb_kernel_t tb_pick_dkv(int flags) {
    switch (flags) {
        case 0: return k_t5_attn_bwd_dkv<DKV, 0>;
        case 1: return k_t5_attn_bwd_dkv<DKV, 1>;
        case 2: return k_t5_attn_bwd_dkv<DKV, 2>;
        case 3: return k_t5_attn_bwd_dkv<DKV, 3>;
        case 4: return k_t5_attn_bwd_dkv<DKV, 4>;
        case 5: return k_t5_attn_bwd_dkv<DKV, 5>;
        case 6: return k_t5_attn_bwd_dkv<DKV, 6>;
        default: return k_t5_attn_bwd_dkv<DKV, 7>;
    }
}
template <int DKV, bool DBIAS>
static tb_kernel_t tb_pick_dq(int flags) {
    switch (flags) {
        case 0: return k_t5_attn_bwd_dq<DKV, 0, DBIAS>;
        case 1: return k_t5_attn_bwd_dq<DKV, 1, DBIAS>;
        case 2: return k_t5_attn_bwd_dq<DKV, 2, DBIAS>;
        case 3: return k_t5_attn_bwd_dq<DKV, 3, DBIAS>;
        case 4: return k_t5_attn_bwd_dq<DKV, 4, DBIAS>;
        case 5: return k_t5_attn_bwd_dq<DKV, 5, DBIAS>;
        case 6: return k_t5_attn_bwd_dq<DKV, 6, DBIAS>;
        default: return k_t5_attn_bwd_dq<DKV, 7, DBIAS>;
    }
}

// Two operands with the SAME strides and sizes, the second `rem` elements after the first: do two of
// their rows of d elements share an element?  s / n: the strides of the dimensions with more than
// one index, largest first, nested (each at least the extent of the ones after it: ta_strides_ok's
// dense rule), so the multiple of s[0] in a difference is its floor quotient or the next one.
static bool tb_rows_meet(const int64_t* s, const int64_t* n, int cnt, int64_t d, int64_t rem) {
    if (cnt == 0) return rem > -d && rem < d;
    int64_t c0 = rem / s[0];
    if (rem % s[0] < 0) --c0;
    for (int64_t c = c0; c <= c0 + 1; ++c)
        if (c > -n[0] && c < n[0] && tb_rows_meet(s + 1, n + 1, cnt - 1, d, rem - c * s[0])) return true;
    return false;
}

static bool tb_sizes_ok(int64_t B, int64_t nH, int64_t Tq) {
    const int64_t lim = int64_t(1) << 30;
    return B >= 1 && nH >= 1 && Tq >= 1 && B <= lim && nH <= lim && Tq <= lim;
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_attention_bwd_tiles(int* dq_q_tile, int* dq_kv_tile, int* dkv_k_tile, int* dkv_q_tile) {
    if (dq_q_tile) *dq_q_tile = kTbDqQTile;
    if (dq_kv_tile) *dq_kv_tile = kTbDqKVTile;
    if (dkv_k_tile) *dkv_k_tile = kTbKvKTile;
    if (dkv_q_tile) *dkv_q_tile = kTbKvQTile;
    return TRLX_OK;
}

extern "C" int64_t trlx_t5_attention_bwd_workspace_bytes(int64_t B, int64_t n_heads, int64_t Tq) {
    if (!tb_sizes_ok(B, n_heads, Tq)) return -1;
    int64_t n;
    if (__builtin_mul_overflow(B, n_heads, &n) || __builtin_mul_overflow(n, Tq, &n) || n > (int64_t(1) << 58)) return -1;
    return (4 * n + 255) / 256 * 256;   // delta, fp32 [B, nH, Tq]
}

extern "C" int trlx_t5_attention_bwd(const TrlxT5AttentionBwdArgs* a, void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 attention bwd: NULL arguments");
    TRLX_REQUIRE(a->dtype == TRLX_BF16, TRLX_ERR_ARG, "t5 attention bwd: dtype %d (bf16 only)", a->dtype);
    TRLX_REQUIRE(a->d_kv == 64 || a->d_kv == 128, TRLX_ERR_ARG, "t5 attention bwd: d_kv %lld (64 and 128 only)",
                 (long long)a->d_kv);
    TRLX_REQUIRE(tb_sizes_ok(a->B, a->n_heads, a->Tq) && a->S >= 1 && a->S <= (int64_t(1) << 30), TRLX_ERR_ARG,
                 "t5 attention bwd: B %lld, heads %lld, Tq %lld, S %lld (each in [1, 2^30])", (long long)a->B,
                 (long long)a->n_heads, (long long)a->Tq, (long long)a->S);
    const int64_t nqb = (a->Tq + kTbDqQTile - 1) / kTbDqQTile;
    const int64_t nkb = (a->S + kTbKvKTile - 1) / kTbKvKTile;
    const int64_t nrb = (a->Tq + 31) / 32;            // delta: one wave per 32 rows
    const int64_t wpb = kTbThreads / kWave;
    int64_t bh, grid_q, grid_k, nwaves;
    TRLX_REQUIRE(!__builtin_mul_overflow(a->B, a->n_heads, &bh) && !__builtin_mul_overflow(bh, nqb, &grid_q) &&
                     !__builtin_mul_overflow(bh, nkb, &grid_k) && !__builtin_mul_overflow(bh, nrb, &nwaves) &&
                     grid_q <= 0x7fffffffLL && grid_k <= 0x7fffffffLL && (nwaves + wpb - 1) / wpb <= 0x7fffffffLL,
                 TRLX_ERR_ARG, "t5 attention bwd: B * heads * blocks = %lld * %lld * max(%lld, %lld) exceeds the grid",
                 (long long)a->B, (long long)a->n_heads, (long long)nqb, (long long)nkb);
    TRLX_REQUIRE(!a->causal || a->Tq == a->S, TRLX_ERR_ARG, "t5 attention bwd: causal needs Tq == S, got %lld and %lld",
                 (long long)a->Tq, (long long)a->S);
    TRLX_REQUIRE(a->q && a->k && a->v && a->out, TRLX_ERR_ARG, "t5 attention bwd: NULL q / k / v / out");
    TRLX_REQUIRE(a->dout && a->lse && a->dq && a->dk && a->dv, TRLX_ERR_ARG,
                 "t5 attention bwd: NULL dout / lse / dq / dk / dv");
    TRLX_REQUIRE(ta_aligned16(a->q) && ta_aligned16(a->k) && ta_aligned16(a->v) && ta_aligned16(a->out) &&
                     ta_aligned16(a->dout) && ta_aligned16(a->dq) && ta_aligned16(a->dk) && ta_aligned16(a->dv),
                 TRLX_ERR_ARG, "t5 attention bwd: q, k, v, out, dout, dq, dk and dv must be 16-byte aligned");
    struct Op {
        const char* name;
        const void* base;
        int64_t T, sb, st, sh;
        bool dense;
        int64_t span;
    };
    Op ops[8] = {{"q", a->q, a->Tq, a->q_stride_b, a->q_stride_t, a->q_stride_h, false, 0},
                 {"k", a->k, a->S, a->k_stride_b, a->k_stride_t, a->k_stride_h, false, 0},
                 {"v", a->v, a->S, a->v_stride_b, a->v_stride_t, a->v_stride_h, false, 0},
                 {"out", a->out, a->Tq, a->o_stride_b, a->o_stride_t, a->o_stride_h, false, 0},
                 {"dout", a->dout, a->Tq, a->do_stride_b, a->do_stride_t, a->do_stride_h, false, 0},
                 {"dq", a->dq, a->Tq, a->dq_stride_b, a->dq_stride_t, a->dq_stride_h, true, 0},
                 {"dk", a->dk, a->S, a->dk_stride_b, a->dk_stride_t, a->dk_stride_h, true, 0},
                 {"dv", a->dv, a->S, a->dv_stride_b, a->dv_stride_t, a->dv_stride_h, true, 0}};
    for (Op& op : ops) {
        TRLX_REQUIRE(ta_strides_ok(a->B, op.T, a->n_heads, a->d_kv, op.sb, op.st, op.sh, op.dense, &op.span), TRLX_ERR_ARG,
                     "t5 attention bwd: %s strides %lld / %lld / %lld (multiples of 8, rows of d_kv apart%s)", op.name,
                     (long long)op.sb, (long long)op.st, (long long)op.sh, op.dense ? " that do not overlap" : "");
    }
    // A written operand may not share an element with any other operand.  Address ranges apart: fine.
    // Ranges that interleave (the slices of one fused buffer) are taken only between operands of the
    // same sizes and strides, where the rows can be told apart exactly.
    for (int x = 5; x < 8; ++x)
        for (int y = 0; y < x; ++y) {
            const Op &X = ops[x], &Y = ops[y];
            const uintptr_t x0 = reinterpret_cast<uintptr_t>(X.base), y0 = reinterpret_cast<uintptr_t>(Y.base);
            if (x0 + 2 * uintptr_t(X.span + 1) <= y0 || y0 + 2 * uintptr_t(Y.span + 1) <= x0) continue;
            const int64_t cnt[3] = {a->B, X.T, a->n_heads}, xs[3] = {X.sb, X.st, X.sh}, ys[3] = {Y.sb, Y.st, Y.sh};
            int64_t s[3], n[3];
            int m = 0;
            bool same = X.T == Y.T;
            for (int i = 0; i < 3; ++i) {
                if (cnt[i] == 1) continue;
                same = same && xs[i] == ys[i];
                int j = m++;
                for (; j > 0 && s[j - 1] < xs[i]; --j) s[j] = s[j - 1], n[j] = n[j - 1];
                s[j] = xs[i], n[j] = cnt[i];
            }
            const int64_t rem = (int64_t(y0) - int64_t(x0)) / 2;
            TRLX_REQUIRE(same && !tb_rows_meet(s, n, m, a->d_kv, rem), TRLX_ERR_ARG,
                         "t5 attention bwd: %s overlaps %s (a written operand shares no element with another; interleaved "
                         "address ranges need equal sizes and strides)", X.name, Y.name);
        }
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(a->lse) & 3u) == 0, TRLX_ERR_ARG, "t5 attention bwd: lse not aligned to 4 bytes");
    TRLX_REQUIRE(!a->bias_by_offset || (reinterpret_cast<uintptr_t>(a->bias_by_offset) & 3u) == 0, TRLX_ERR_ARG,
                 "t5 attention bwd: bias_by_offset not aligned to 4 bytes");
    TRLX_REQUIRE(!a->dbias || (reinterpret_cast<uintptr_t>(a->dbias) & 3u) == 0, TRLX_ERR_ARG,
                 "t5 attention bwd: dbias not aligned to 4 bytes");
    TRLX_REQUIRE(!a->key_mask || (reinterpret_cast<uintptr_t>(a->key_mask) & 7u) == 0, TRLX_ERR_ARG,
                 "t5 attention bwd: key_mask not aligned to 8 bytes");
    const int64_t need = trlx_t5_attention_bwd_workspace_bytes(a->B, a->n_heads, a->Tq);
    TRLX_REQUIRE(need > 0 && a->workspace && (reinterpret_cast<uintptr_t>(a->workspace) & 3u) == 0 &&
                     a->workspace_bytes >= need,
                 TRLX_ERR_ARG, "t5 attention bwd: workspace of %lld bytes, %lld needed (4-byte aligned)",
                 (long long)a->workspace_bytes, (long long)need);

    TbArgs k = {};
    k.q = static_cast<const uint16_t*>(a->q);
    k.k = static_cast<const uint16_t*>(a->k);
    k.v = static_cast<const uint16_t*>(a->v);
    k.o = static_cast<const uint16_t*>(a->out);
    k.dout = static_cast<const uint16_t*>(a->dout);
    k.dq = static_cast<uint16_t*>(a->dq);
    k.dk = static_cast<uint16_t*>(a->dk);
    k.dv = static_cast<uint16_t*>(a->dv);
    k.lse = a->lse;
    k.delta = static_cast<float*>(a->workspace);
    k.bias = a->bias_by_offset;
    k.mask = a->key_mask;
    k.dbias = a->dbias;
    // a stride that is never multiplied by a non-zero index is not read
    const bool b1 = a->B == 1, q1 = a->Tq == 1, s1 = a->S == 1, h1 = a->n_heads == 1;
    k.q_sb = b1 ? 0 : a->q_stride_b, k.q_st = q1 ? 0 : a->q_stride_t, k.q_sh = h1 ? 0 : a->q_stride_h;
    k.k_sb = b1 ? 0 : a->k_stride_b, k.k_st = s1 ? 0 : a->k_stride_t, k.k_sh = h1 ? 0 : a->k_stride_h;
    k.v_sb = b1 ? 0 : a->v_stride_b, k.v_st = s1 ? 0 : a->v_stride_t, k.v_sh = h1 ? 0 : a->v_stride_h;
    k.o_sb = b1 ? 0 : a->o_stride_b, k.o_st = q1 ? 0 : a->o_stride_t, k.o_sh = h1 ? 0 : a->o_stride_h;
    k.do_sb = b1 ? 0 : a->do_stride_b, k.do_st = q1 ? 0 : a->do_stride_t, k.do_sh = h1 ? 0 : a->do_stride_h;
    k.dq_sb = b1 ? 0 : a->dq_stride_b, k.dq_st = q1 ? 0 : a->dq_stride_t, k.dq_sh = h1 ? 0 : a->dq_stride_h;
    k.dk_sb = b1 ? 0 : a->dk_stride_b, k.dk_st = s1 ? 0 : a->dk_stride_t, k.dk_sh = h1 ? 0 : a->dk_stride_h;
    k.dv_sb = b1 ? 0 : a->dv_stride_b, k.dv_st = s1 ? 0 : a->dv_stride_t, k.dv_sh = h1 ? 0 : a->dv_stride_h;
    k.nH = int(a->n_heads);
    k.Tq = int(a->Tq);
    k.S = int(a->S);
    hipStream_t st = (hipStream_t)stream;
    if (a->dbias) {
        const hipError_t e = hipMemsetAsync(a->dbias, 0, size_t(a->n_heads) * size_t(a->Tq + a->S - 1) * 4, st);
        TRLX_REQUIRE(e == hipSuccess, TRLX_ERR_LAUNCH,"t5 attention bwd: zeroing dbias: %s", hipGetErrorString(e));
    }
    const int flags = (a->bias_by_offset ? kTaBias : 0) | (a->key_mask ? kTaMask : 0) | (a->causal ? kTaCausal : 0);
    {
        auto fn = a->d_kv == 64 ? k_t5_attn_bwd_delta<64> : k_t5_attn_bwd_delta<128>;
        hipLaunchKernelGGL(fn, dim3(unsigned((nwaves + wpb - 1) / wpb)), dim3(kTbThreads), 0, st, k, int(nrb), nwaves);
        const int rc = check_launch("k_t5_attn_bwd_delta");
        if (rc != TRLX_OK) return rc;
    }
    {
        k.nblk = int(nkb);
        tb_kernel_t fn = a->d_kv == 64 ? tb_pick_dkv<64>(flags) : tb_pick_dkv<128>(flags);
        hipLaunchKernelGGL(fn, dim3(unsigned(grid_k)), dim3(kTbThreads), 0, st, k);
        const int rc = check_launch("k_t5_attn_bwd_dkv");
        if (rc != TRLX_OK) return rc;
    }
    k.nblk = int(nqb);
    tb_kernel_t fn = a->dbias ? (a->d_kv == 64 ? tb_pick_dq<64, true>(flags) : tb_pick_dq<128, true>(flags))
                              : (a->d_kv == 64 ? tb_pick_dq<64, false>(flags) : tb_pick_dq<128, false>(flags));
    hipLaunchKernelGGL(fn, dim3(unsigned(grid_q)), dim3(kTbThreads), 0, st, k);
    return check_launch("k_t5_attn_bwd_dq");
}
