// The grouped decode cross-attention on matrix instructions: the G samples of a prompt are the
// query rows of an MFMA tile.  See trlx_t5_decode_attn_group_mma in trlx_t5_amd.h.  The arguments
// and their meaning are trlx_t5_decode_attn_group's (t5_decode_attn_group.hip), bf16 only.
//
// One workgroup of W waves = one (prompt, head, tile of kGmQ = 16 queries), grid (P * nH,
// ceil(G / 16)).  The S keys are cut into blocks of kGmKeys = 32; wave w walks blocks w, w + W, ...
// on its own: nothing in the key loop is shared between waves, so the loop has no workgroup barrier.
//
// Scores, S^T = K·Q^T on v_mfma_f32_16x16x32_bf16.  A = 16 key rows: lane (c = lane & 15,
// g = lane >> 4) loads the 16-byte vector K[key c][32 kk + 8 g ..] straight from global memory, K
// never passes through LDS.  B = Q^T, lane (c, g) holds Q[query c][32 kk + 8 g ..], loaded once
// (d_kv / 32 fragments).  The result has the QUERY on the lane (c) and keys 4 g .. 4 g + 3 of the
// 16 in the lane's four registers: a query's running max, sum and rescale factor are one value per
// lane, and a maximum over keys is the lane's own registers and two exchanges (lanes 16 and 32
// apart).
//
// P·V, O^T[d x 16] += V^T[d x 32]·P^T[32 x 16].  The two 16-key score blocks of a 32-key block (keys
// 0..15 and 16..31, both in natural order) leave lane (c, g) with P of keys 4 g + r and 16 + 4 g + r,
// r = 0..3.  Those eight values, rounded to bf16 un-normalised, ARE the B operand if k-slot 8 g + e
// of the instruction stands for key 4 g + e (e < 4) or 16 + 4 g + e - 4: P never leaves registers.
// The A operand V^T has to come in the same slot order: the wave's 32 V rows go global -> registers
// -> LDS row-major, and lane (c, g) takes column 16 db + c of rows 4 g .. 4 g + 3 and of rows
// 16 + 4 g .. with two ds_read_b64_tr_b16.  Putting the permutation on the V side (not, as
// t5_attention.hip's 32x32 tile has to, on the order of the key rows) keeps every K load in
// natural order and makes the 32 lanes of a half-wave read eight consecutive rows, 32 bytes each,
// which the row stride 2 d_kv + 32 spreads over all 64 banks.
//
// LDS.  A wave owns one 32-row V region and nothing else.  The next block's K and V are loaded
// into registers under the current block's MFMAs; those registers are the second buffer.  A second
// LDS buffer would buy nothing: the LDS operations of one wave execute in order, so block j + W's
// writes cannot pass block j's transposed reads, and half the LDS keeps two workgroups on a CU.
// After the loop a wave parks (m, l, O^T) in its own region, one barrier, and 16 * d_kv / 8 threads
// merge the waves in wave order against the common maximum, divide, round once and store 16 bytes.
//
// Keys that do not count.  A lane-ballot of the block's 32 keys (in range, key_mask != 0) is the
// wave-uniform word every decision is taken from: a block without a live key is skipped and none of
// its rows is read; a dead row's K and V vectors are zeros in registers instead of loads, and its
// score is -inf, so a NaN in a masked row reaches no MFMA.  Queries past G and dead queries have
// zero Q fragments (their rows are not read); MFMA columns are independent, so a row's bits depend
// on its own q, the prompt's keys, values and mask, and S, and on nothing else.
#include "t5_attention.h"
#include "t5_decode_group_check.h"

#ifndef TRLX_T5GM_WAVES_D64
#define TRLX_T5GM_WAVES_D64 8
#endif
#ifndef TRLX_T5GM_WAVES_D128
#define TRLX_T5GM_WAVES_D128 8
#endif

namespace trlx {

constexpr int kGmQ = 16;      // queries per workgroup: the N of the MFMA
constexpr int kGmKeys = 32;   // keys per block: the K of the P·V MFMA, two score blocks
constexpr int kGmWaves64 = TRLX_T5GM_WAVES_D64, kGmWaves128 = TRLX_T5GM_WAVES_D128;

typedef float gm_f32x4 __attribute__((ext_vector_type(4)));

struct T5GmArgs {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    const int64_t* mask;    // [P, S] or NULL (MASKED = false)
    const int64_t* live;    // [P * G] or NULL (LIVE = false)
    uint16_t* out;
    int64_t ldq;
    int64_t k_sp, k_sh, k_ss, v_sp, v_sh, v_ss;   // element strides over (p, h, s)
    int nH, G, S;
};

__device__ __forceinline__ ta_bf16x8 gm_frag(const vec4u& x) { return __builtin_bit_cast(ta_bf16x8, x); }

// blockIdx.x = p * nH + h, blockIdx.y = the tile: queries g0 = 16 * tile ... g0 + nq - 1 of prompt p.
// `on` has one bit per query of the tile: set for a query that exists and, with LIVE, whose live word
// is non-zero.  It is the same word in every wave.  on == 0: zeros to the tile's out rows and out,
// before any barrier and before any address into q, K, V or the mask is formed.
template <int DKV, bool MASKED, bool LIVE, int W>
__global__ __launch_bounds__(W* kWave) void k_t5_decode_attn_group_mma(const T5GmArgs a) {
    constexpr int CPR = DKV / 8;                     // 16-byte chunks per row
    constexpr int KK = DKV / 32;                     // k-steps of K·Q^T
    constexpr int DB = DKV / 16;                     // 16-row blocks of O^T
    constexpr int NV = kGmKeys * CPR / kWave;        // V chunks per lane and block
    constexpr int VS = 2 * DKV + 32;                 // V row stride in LDS, bytes
    constexpr int PS = DKV + 4;                      // parked O row stride, floats
    constexpr int kRegion = kGmKeys * VS;            // one wave's LDS, bytes
    constexpr int kThreads = W * kWave;
    static_assert(DKV % 32 == 0 && NV * kWave == kGmKeys * CPR && kWave % CPR == 0, "tile geometry");
    static_assert((kGmQ * PS + 2 * kGmQ) * 4 <= kRegion && PS % 4 == 0, "a wave parks its state in its V region");
    static_assert(kGmQ * CPR <= kThreads && W * kRegion <= 160 * 1024, "merge threads, LDS");
    __shared__ __attribute__((aligned(16))) unsigned char smem[W * kRegion];

    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int c = lane & 15, g = lane >> 4;
    const int ph = blockIdx.x;
    const int p = ph / a.nH, h = ph - p * a.nH;
    const int g0 = int(blockIdx.y) * kGmQ;
    const int nq = a.G - g0 < kGmQ ? a.G - g0 : kGmQ;
    const int64_t b0 = int64_t(p) * a.G + g0;        // the tile's first row of q / out / live
    bool mine = lane < nq;                           // lane i < 16 answers for query i
    if constexpr (LIVE) {
        if (mine) mine = a.live[b0 + lane] != 0;
    }
    const unsigned on = unsigned(__ballot(mine));
    if constexpr (LIVE) {
        if (on == 0) {   // block-uniform
            for (int i = tid; i < nq * CPR; i += kThreads)
                *reinterpret_cast<vec4u*>(a.out + ((b0 + i / CPR) * a.nH + h) * DKV + (i % CPR) * 8) = vec4u_make(0, 0, 0, 0);
            return;
        }
    }

    // Q^T fragments: lane (c, g) holds Q[query c][32 kk + 8 g + 0..7], zeros for a query that is off
    vec4u qf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        qf[kk] = vec4u_make(0, 0, 0, 0);
        if ((on >> c) & 1u)
            qf[kk] = *reinterpret_cast<const vec4u*>(a.q + (b0 + c) * a.ldq + h * DKV + 32 * kk + 8 * g);
    }
    const uint16_t* K = a.k + int64_t(p) * a.k_sp + int64_t(h) * a.k_sh;
    const uint16_t* V = a.v + int64_t(p) * a.v_sp + int64_t(h) * a.v_sh;
    const int64_t* mask = MASKED ? a.mask + int64_t(p) * a.S : nullptr;

    // block j into registers: the word of its live keys, the live rows' K fragments and V chunks
    vec4u kr[2][KK], vr[NV];
    unsigned lmN = 0;
    auto prefetch = [&](int j) __attribute__((always_inline)) {
        const int key0 = j * kGmKeys;
        bool alive = lane < kGmKeys && key0 + lane < a.S;
        if (MASKED) {
            if (alive) alive = mask[key0 + lane] != 0;
        }
        lmN = unsigned(__ballot(alive));
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int row = 16 * blk + c;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                kr[blk][kk] = vec4u_make(0, 0, 0, 0);
                if ((lmN >> row) & 1u)
                    kr[blk][kk] = *reinterpret_cast<const vec4u*>(K + int64_t(key0 + row) * a.k_ss + 32 * kk + 8 * g);
            }
        }
#pragma unroll
        for (int n = 0; n < NV; ++n) {
            const int cid = lane + kWave * n;
            const int row = cid / CPR, ch = cid % CPR;
            vr[n] = vec4u_make(0, 0, 0, 0);
            if ((lmN >> row) & 1u) vr[n] = *reinterpret_cast<const vec4u*>(V + int64_t(key0 + row) * a.v_ss + ch * 8);
        }
    };

    float m = -INFINITY, l = 0.f;   // l: this lane's keys only, summed over the four g at the end
    gm_f32x4 O[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) O[db] = gm_f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned char* sV = smem + wave * kRegion;
    // lane 4 q + x of a 16-lane group addresses row q, columns 4 x .. 4 x + 3 of a 4-row x 16-column
    // block and receives its column c of the 4 rows; group g takes rows 4 g .. of each half
    const unsigned char* vp = sV + (4 * g + (c >> 2)) * VS + 4 * (c & 3) * 2;

    const int nblk = (a.S + kGmKeys - 1) / kGmKeys;
    if (wave < nblk) prefetch(wave);
#pragma unroll 1
    for (int j = wave; j < nblk; j += W) {
        const unsigned lm = lmN;
        vec4u kc[2][KK];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) kc[blk][kk] = kr[blk][kk];
        if (lm) {   // wave-uniform
#pragma unroll
            for (int n = 0; n < NV; ++n) {
                const int cid = lane + kWave * n;
                *reinterpret_cast<vec4u*>(sV + (cid / CPR) * VS + (cid % CPR) * 16) = vr[n];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (j + W < nblk) prefetch(j + W);
        if (!lm) continue;

        // S^T = K·Q^T: two blocks of 16 keys
        gm_f32x4 sacc[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            sacc[blk] = gm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                sacc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gm_frag(kc[blk][kk]), gm_frag(qf[kk]), sacc[blk], 0, 0, 0);
        }
        // dead keys, the block's max per query
        float mx = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool dead = !((lm >> (16 * blk + 4 * g + r)) & 1u);
                const float s = dead ? -INFINITY : sacc[blk][r];
                sacc[blk][r] = s;
                mx = fmaxf(mx, s);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
        mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
        const float mn = fmaxf(m, mx);
        const float mu = mn == -INFINITY ? 0.f : mn;   // no live key yet: every p is exp2(-inf) = 0
        const float sc = exp2_fast((m - mu) * kLog2e);
        m = mn;
        float ps = 0.f;
        ta_bf16x8 pf;   // k-slots 8 g + e: keys 4 g + e (e < 4) and 16 + 4 g + e - 4
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pr = exp2_fast((sacc[blk][r] - mu) * kLog2e);
                ps += pr;
                pf[4 * blk + r] = static_cast<__bf16>(pr);
            }
        l = l * sc + ps;
        // O^T = O^T * sc + V^T·P^T
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int r = 0; r < 4; ++r) O[db][r] *= sc;
            const ta_s16x4 v0 = ta_tr_read(vp + 32 * db), v1 = ta_tr_read(vp + 16 * VS + 32 * db);
            const ta_bf16x8 vf = __builtin_bit_cast(ta_bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
            O[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, O[db], 0, 0, 0);
        }
    }

    // park (m, l, O^T) in the wave's own region: O as [query][d], then m[16], l[16]
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
    {
        float* park = reinterpret_cast<float*>(sV);
#pragma unroll
        for (int db = 0; db < DB; ++db) *reinterpret_cast<gm_f32x4*>(park + c * PS + 16 * db + 4 * g) = O[db];
        if (g == 0) {
            park[kGmQ * PS + c] = m;
            park[kGmQ * PS + kGmQ + c] = l;
        }
    }
    __syncthreads();
    // merge: one thread per (query, 8 columns), the waves in wave order
    const int qi = tid / CPR, ch = tid - qi * CPR;
    if (qi >= nq) return;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
    if ((on >> qi) & 1u) {
        float M = -INFINITY;
        for (int w = 0; w < W; ++w) M = fmaxf(M, reinterpret_cast<const float*>(smem + w * kRegion)[kGmQ * PS + qi]);
        float L = 0.f;
        for (int w = 0; w < W; ++w) {
            const float* park = reinterpret_cast<const float*>(smem + w * kRegion);
            const float mw = park[kGmQ * PS + qi];
            if (mw == -INFINITY) continue;   // a wave that saw no live key
            const float wgt = exp2_fast((mw - M) * kLog2e);
            L += park[kGmQ * PS + kGmQ + qi] * wgt;
            const gm_f32x4 x0 = *reinterpret_cast<const gm_f32x4*>(park + qi * PS + 8 * ch);
            const gm_f32x4 x1 = *reinterpret_cast<const gm_f32x4*>(park + qi * PS + 8 * ch + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] += x0[e] * wgt;
                o[4 + e] += x1[e] * wgt;
            }
        }
        const bool any = L > 0.f || L != L;   // no live key at all (a fully masked prompt): zeros
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = any ? o[e] / L : 0.f;
    }
    *reinterpret_cast<vec4u*>(a.out + ((b0 + qi) * a.nH + h) * DKV + 8 * ch) =
        vec4u_make(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7]));   // dead: zeros
}

typedef void (*t5_gm_kernel_t)(const T5GmArgs);
template <int DKV, int W>
static t5_gm_kernel_t t5_gm_pick(bool masked, bool live) {
    if (live)
        return masked ? k_t5_decode_attn_group_mma<DKV, true, true, W> : k_t5_decode_attn_group_mma<DKV, false, true, W>;
    return masked ? k_t5_decode_attn_group_mma<DKV, true, false, W> : k_t5_decode_attn_group_mma<DKV, false, false, W>;
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_decode_attn_group_mma_waves(int64_t d_kv) {
    return d_kv == 64 ? kGmWaves64 : d_kv == 128 ? kGmWaves128 : 0;
}

extern "C" int trlx_t5_decode_attn_group_mma(const TrlxT5DecodeAttnGroupArgs* a, void* stream) {
    T5GroupChecked c;   // the grid is (P * heads, ceil(G / 16))
    const int rc = t5_group_check(a, "t5 grouped mma decode attention", false, false, kGmQ, &c);
    if (rc) return rc;
    T5GmArgs k = {};
    k.q = static_cast<const uint16_t*>(a->q);
    k.k = static_cast<const uint16_t*>(a->k);
    k.v = static_cast<const uint16_t*>(a->v);
    k.mask = a->key_mask;
    k.live = a->live;
    k.out = static_cast<uint16_t*>(a->out);
    k.ldq = c.ldq;
    k.k_sp = c.st[0], k.k_sh = c.st[1], k.k_ss = c.st[2];
    k.v_sp = c.st[3], k.v_sh = c.st[4], k.v_ss = c.st[5];
    k.nH = int(a->n_heads);
    k.G = int(a->G);
    k.S = int(a->S);
    const bool masked = a->key_mask != nullptr, live = a->live != nullptr;
    const dim3 grid(unsigned(a->P * a->n_heads), unsigned(c.tiles));
    if (a->d_kv == 64)
        hipLaunchKernelGGL((t5_gm_pick<64, kGmWaves64>(masked, live)), grid, dim3(kGmWaves64 * kWave), 0, (hipStream_t)stream, k);
    else
        hipLaunchKernelGGL((t5_gm_pick<128, kGmWaves128>(masked, live)), grid, dim3(kGmWaves128 * kWave), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn_group_mma");
}
