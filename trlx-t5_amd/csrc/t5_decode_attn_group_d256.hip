// The grouped decode cross-attention on matrix instructions at d_kv 256 (the UL2 head size), with
// the encoder keys split across workgroups inside the same kernel.  See
// trlx_t5_decode_attn_group_d256 in trlx_t5_amd.h.  The arguments and their meaning are
// trlx_t5_decode_attn_group's (t5_decode_attn_group.hip), bf16 only.
//
// Why a kernel of its own.  k_t5_decode_attn_group_mma (t5_decode_attn_group_mma.hip) at 256 with
// its 8 waves needs 256 VGPRs and 384 bytes of scratch a lane and 139,264 bytes of LDS; with 4
// waves it fits (256 VGPRs + ~148 AGPRs at one wave a SIMD, 69,632 bytes) but its merge wants
// 16 * 256 / 8 = 512 threads of 256, and its grid, already 16 times smaller than the plain call's
// once samples share a tile, leaves most of the chip idle at UL2 rollouts (8 prompts x 16 heads =
// 128 workgroups on 256 CUs).  So: 4 waves, one a SIMD, a merge in two passes, and a third grid
// dimension over ranges of the keys.
//
// One workgroup of 4 waves = one (prompt, head, tile of kGdQ = 16 queries, range x of the keys),
// grid (P * nH, ceil(G / 16), ranges).  The S keys are cut into nblk = ceil(S / 32) blocks of 32;
// with cb = ceil(nblk / X) range x holds blocks [x cb, min(nblk, (x + 1) cb)) and wave w walks blocks
// x cb + w, + 4, ... on its own: nothing in the key loop is shared between waves, so the loop has
// no workgroup barrier.
//
// The arithmetic per block is that of the 64 / 128 kernel.  Scores, S^T = K·Q^T on
// v_mfma_f32_16x16x32_bf16: lane (c = lane & 15, g = lane >> 4) loads the 16-byte vector
// K[key c][32 kk + 8 g ..] straight from global memory as the A operand (K never passes through
// LDS) and holds Q[query c][32 kk + 8 g ..] as B, loaded once (8 fragments).  The result has the
// query on the lane and keys 4 g .. 4 g + 3 of the 16 in its four registers, so a query's running
// max, sum and rescale factor are one value a lane.  The two 16-key score blocks leave lane (c, g)
// with P of keys 4 g + r and 16 + 4 g + r; rounded to bf16 un-normalised those eight values ARE the
// B operand of O^T[256 x 16] += V^T[256 x 32]·P^T[32 x 16] when k-slot 8 g + e stands for key 4 g + e
// (e < 4) or 16 + 4 g + e - 4.  V^T comes in that slot order out of the wave's own LDS region (32 rows,
// row stride 2 * 256 + 32 bytes) through two ds_read_b64_tr_b16 per 16 output rows.
//
// Registers (one wave a SIMD: 512 a lane; the kernels take 256 VGPRs + 148 or 149 AGPRs, no
// scratch).  Q fragments 32, the next block's K 64 and V 64 (loaded under the current block's
// MFMAs: they are the second buffer), the current block's K 64, O^T 64 accumulators.  A form for
// two workgroups a CU (launch bounds (256, 2), the next K loaded after the scores so that no
// second K copy lives) compiled to 168 bytes of scratch a lane and is not built: DESIGN.md.
//
// After the loop a wave parks (m, l, O^T as [16][256] fp32) in its own V region; one barrier; the
// 256 threads cover the 16 x 32 (query, 8 columns) items in two passes, each item adding the four
// waves in wave order against their common maximum.  Without SPLIT the item is divided, rounded
// once and stored; with SPLIT the undivided (M, L, o[256]) of a live query goes to
// workspace[((row * nH + h) * ranges + x) * 258] and k_t5_decode_attn_group_d256_merge combines a
// row's ranges in range order.  No atomics: a row's bits depend on its own q, the prompt's keys,
// values and mask, S and the split, and on nothing else.
//
// Keys that do not count, as in the 64 / 128 kernel: a wave-uniform ballot of the block's live keys
// drives every decision; a block without one is skipped and not read; a dead row's K and V are
// zeros in registers and its score is -inf; off queries have zero Q fragments; a tile with on == 0
// leaves before any address is formed (without SPLIT it writes zeros).
#include "t5_attention.h"
#include "t5_decode_group_check.h"

namespace trlx {

constexpr int kGdD = 256;        // d_kv
constexpr int kGdQ = 16;         // queries per workgroup: the N of the MFMA
constexpr int kGdKeys = 32;      // keys per block: the K of the P·V MFMA, two score blocks
constexpr int kGdWaves = 4;      // one a SIMD
constexpr int kGdThreads = kGdWaves * kWave;
constexpr int kGdMaxSplits = 8;
constexpr int kGdRec = kGdD + 2;   // a workspace record: M, L, o[256]

typedef float gd_f32x4 __attribute__((ext_vector_type(4)));

struct T5GdArgs {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    const int64_t* mask;    // [P, S] or NULL (MASKED = false)
    const int64_t* live;    // [P * G] or NULL (LIVE = false)
    uint16_t* out;
    float* ws;              // [P * G, nH, ranges, 258] (SPLIT and the merge)
    int64_t ldq;
    int64_t k_sp, k_sh, k_ss, v_sp, v_sh, v_ss;   // element strides over (p, h, s)
    int nH, G, S;
    int cb, ranges;         // blocks a range, ranges launched
    int rows;               // P * G
};

__device__ __forceinline__ ta_bf16x8 gd_frag(const vec4u& x) { return __builtin_bit_cast(ta_bf16x8, x); }

// blockIdx.x = p * nH + h, blockIdx.y = the tile (queries g0 = 16 * tile ... g0 + nq - 1 of prompt
// p), blockIdx.z = the key range (0 without SPLIT).  `on` has one bit per query of the tile: set
// for a query that exists and, with LIVE, whose live word is non-zero; the same word in every wave.
template <bool MASKED, bool LIVE, bool SPLIT>
__global__ __launch_bounds__(kGdThreads, 1) void k_t5_decode_attn_group_d256(const T5GdArgs a) {
    constexpr int CPR = kGdD / 8;                     // 16-byte chunks per row
    constexpr int KK = kGdD / 32;                     // k-steps of K·Q^T
    constexpr int DB = kGdD / 16;                     // 16-row blocks of O^T
    constexpr int NV = kGdKeys * CPR / kWave;         // V chunks per lane and block
    constexpr int VS = 2 * kGdD + 32;                 // V row stride in LDS, bytes
    constexpr int PS = kGdD + 4;                      // parked O row stride, floats
    constexpr int kRegion = kGdKeys * VS;             // one wave's LDS, bytes
    static_assert(NV * kWave == kGdKeys * CPR && kWave % CPR == 0, "tile geometry");
    static_assert((kGdQ * PS + 2 * kGdQ) * 4 <= kRegion && PS % 4 == 0, "a wave parks its state in its V region");
    static_assert(kGdQ * CPR == 2 * kGdThreads && kGdWaves * kRegion <= 80 * 1024, "two merge passes, LDS");
    __shared__ __attribute__((aligned(16))) unsigned char smem[kGdWaves * kRegion];

    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int c = lane & 15, g = lane >> 4;
    const int ph = blockIdx.x;
    const int p = ph / a.nH, h = ph - p * a.nH;
    const int g0 = int(blockIdx.y) * kGdQ;
    const int nq = a.G - g0 < kGdQ ? a.G - g0 : kGdQ;
    const int64_t b0 = int64_t(p) * a.G + g0;        // the tile's first row of q / out / live / the workspace
    bool mine = lane < nq;                           // lane i < 16 answers for query i
    if constexpr (LIVE) {
        if (mine) mine = a.live[b0 + lane] != 0;
    }
    const unsigned on = unsigned(__ballot(mine));
    if constexpr (LIVE) {
        if (on == 0) {   // block-uniform
            if constexpr (!SPLIT)
                for (int i = tid; i < nq * CPR; i += kGdThreads)
                    *reinterpret_cast<vec4u*>(a.out + ((b0 + i / CPR) * a.nH + h) * kGdD + (i % CPR) * 8) = vec4u_make(0, 0, 0, 0);
            return;
        }
    }

    // Q^T fragments: lane (c, g) holds Q[query c][32 kk + 8 g + 0..7], zeros for a query that is off
    vec4u qf[KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        qf[kk] = vec4u_make(0, 0, 0, 0);
        if ((on >> c) & 1u)
            qf[kk] = *reinterpret_cast<const vec4u*>(a.q + (b0 + c) * a.ldq + int64_t(h) * kGdD + 32 * kk + 8 * g);
    }
    const uint16_t* K = a.k + int64_t(p) * a.k_sp + int64_t(h) * a.k_sh;
    const uint16_t* V = a.v + int64_t(p) * a.v_sp + int64_t(h) * a.v_sh;
    const int64_t* mask = MASKED ? a.mask + int64_t(p) * a.S : nullptr;

    // block j into registers: the word of its live keys, then the live rows' K fragments and V chunks
    vec4u kr[2][KK], vr[NV];
    unsigned lmN = 0;
    auto prefetch = [&](int j) __attribute__((always_inline)) {
        const int key0 = j * kGdKeys;
        bool alive = lane < kGdKeys && key0 + lane < a.S;
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
    gd_f32x4 O[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) O[db] = gd_f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned char* sV = smem + wave * kRegion;
    // lane 4 q + x of a 16-lane group addresses row q, columns 4 x .. 4 x + 3 of a 4-row x 16-column
    // block and receives its column c of the 4 rows; group g takes rows 4 g .. of each half
    const unsigned char* vp = sV + (4 * g + (c >> 2)) * VS + 4 * (c & 3) * 2;

    // the range's blocks [j0, j1): all of them without SPLIT (the launch passes cb = nblk)
    const int nblk = (a.S + kGdKeys - 1) / kGdKeys;
    const int j0 = SPLIT ? int(blockIdx.z) * a.cb : 0;
    const int j1 = SPLIT ? (nblk - j0 < a.cb ? nblk : j0 + a.cb) : nblk;
    if (j0 + wave < j1) prefetch(j0 + wave);
#pragma unroll 1
    for (int j = j0 + wave; j < j1; j += kGdWaves) {
        const unsigned lm = lmN;
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

        vec4u kc[2][KK];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) kc[blk][kk] = kr[blk][kk];
        if (j + kGdWaves < j1) prefetch(j + kGdWaves);
        if (!lm) continue;

        // S^T = K·Q^T: two blocks of 16 keys
        gd_f32x4 sacc[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            sacc[blk] = gd_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                sacc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gd_frag(kc[blk][kk]), gd_frag(qf[kk]), sacc[blk], 0, 0, 0);
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
        for (int db = 0; db < DB; ++db) *reinterpret_cast<gd_f32x4*>(park + c * PS + 16 * db + 4 * g) = O[db];
        if (g == 0) {
            park[kGdQ * PS + c] = m;
            park[kGdQ * PS + kGdQ + c] = l;
        }
    }
    __syncthreads();
    // merge: two passes of one thread per (query, 8 columns), the waves in wave order
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const int item = pass * kGdThreads + tid;
        const int qi = item / CPR, ch = item - qi * CPR;
        if (qi >= nq) break;
        const bool alive = (on >> qi) & 1u;
        if (SPLIT && !alive) continue;   // a dead query: no state
        float o[8], M = -INFINITY, L = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = 0.f;
        if (alive) {
            for (int w = 0; w < kGdWaves; ++w) M = fmaxf(M, reinterpret_cast<const float*>(smem + w * kRegion)[kGdQ * PS + qi]);
            for (int w = 0; w < kGdWaves; ++w) {
                const float* park = reinterpret_cast<const float*>(smem + w * kRegion);
                const float mw = park[kGdQ * PS + qi];
                if (mw == -INFINITY) continue;   // a wave that saw no live key
                const float wgt = exp2_fast((mw - M) * kLog2e);
                L += park[kGdQ * PS + kGdQ + qi] * wgt;
                const gd_f32x4 x0 = *reinterpret_cast<const gd_f32x4*>(park + qi * PS + 8 * ch);
                const gd_f32x4 x1 = *reinterpret_cast<const gd_f32x4*>(park + qi * PS + 8 * ch + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] += x0[e] * wgt;
                    o[4 + e] += x1[e] * wgt;
                }
            }
        }
        if constexpr (SPLIT) {
            // records are 258 floats apart: 8-byte aligned, so the state goes out as float2
            float* rec = a.ws + (((b0 + qi) * a.nH + h) * a.ranges + int(blockIdx.z)) * kGdRec;
            if (ch == 0) *reinterpret_cast<float2*>(rec) = make_float2(M, L);
#pragma unroll
            for (int e = 0; e < 8; e += 2) *reinterpret_cast<float2*>(rec + 2 + 8 * ch + e) = make_float2(o[e], o[e + 1]);
        } else {
            const bool any = L > 0.f || L != L;   // no live key at all (a fully masked prompt): zeros
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = any ? o[e] / L : 0.f;
            *reinterpret_cast<vec4u*>(a.out + ((b0 + qi) * a.nH + h) * kGdD + 8 * ch) =
                vec4u_make(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7]));   // dead: zeros
        }
    }
}

// Thread t of the grid: columns 8 ch .. 8 ch + 7 of (row, head) = t / 32.  It reads the records the
// part pass of the same call wrote for a live row, and no other.
template <bool LIVE>
__global__ __launch_bounds__(kGdThreads) void k_t5_decode_attn_group_d256_merge(const T5GdArgs a) {
    constexpr int CPR = kGdD / 8;
    const int64_t t = int64_t(blockIdx.x) * kGdThreads + threadIdx.x;
    const int64_t bh = t / CPR;
    if (bh >= int64_t(a.rows) * a.nH) return;
    const int ch = int(t - bh * CPR);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
    bool dead = false;
    if constexpr (LIVE) dead = a.live[bh / a.nH] == 0;
    if (!dead) {
        const float* rec = a.ws + bh * a.ranges * kGdRec;
        float M = -INFINITY, L = 0.f;
        for (int x = 0; x < a.ranges; ++x) M = fmaxf(M, rec[x * kGdRec]);
        for (int x = 0; x < a.ranges; ++x) {
            const float2 ml = *reinterpret_cast<const float2*>(rec + x * kGdRec);
            if (ml.x == -INFINITY) continue;   // a range that held no live key
            const float wgt = exp2_fast((ml.x - M) * kLog2e);
            L += ml.y * wgt;
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const float2 x2 = *reinterpret_cast<const float2*>(rec + x * kGdRec + 2 + 8 * ch + e);
                o[e] += x2.x * wgt;
                o[e + 1] += x2.y * wgt;
            }
        }
        const bool any = L > 0.f || L != L;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = any ? o[e] / L : 0.f;
    }
    *reinterpret_cast<vec4u*>(a.out + bh * kGdD + 8 * ch) =
        vec4u_make(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7]));
}

typedef void (*t5_gd_kernel_t)(const T5GdArgs);
template <bool SPLIT>
static t5_gd_kernel_t t5_gd_pick(bool masked, bool live) {
    if (live)
        return masked ? k_t5_decode_attn_group_d256<true, true, SPLIT> : k_t5_decode_attn_group_d256<false, true, SPLIT>;
    return masked ? k_t5_decode_attn_group_d256<true, false, SPLIT> : k_t5_decode_attn_group_d256<false, false, SPLIT>;
}

// cb = ceil(nblk / X) blocks a range, `ranges` = ceil(nblk / cb) non-empty ranges
static void t5_gd_ranges(int64_t S, int64_t X, int64_t* cb, int64_t* ranges) {
    const int64_t nblk = (S + kGdKeys - 1) / kGdKeys;
    *cb = (nblk + X - 1) / X;
    *ranges = (nblk + *cb - 1) / *cb;
}

}  // namespace trlx

using namespace trlx;

extern "C" int64_t trlx_t5_decode_attn_group_d256_workspace_bytes(int64_t rows, int64_t n_heads, int64_t S, int64_t splits) {
    if (rows < 1 || n_heads < 1 || S < 1 || splits < 2 || splits > kGdMaxSplits) return 0;
    if (rows > 0x7fffffffLL || n_heads > 0x7fffffffLL / 128 || S > 0x7fffffffLL / 128 || rows * n_heads > 0x7fffffffLL) return 0;
    int64_t cb, ranges;
    t5_gd_ranges(S, splits, &cb, &ranges);
    return rows * n_heads * ranges * kGdRec * int64_t(sizeof(float));
}

extern "C" int trlx_t5_decode_attn_group_d256_geometry(int64_t S, int64_t splits, TrlxT5DecodeAttnGroupD256Geometry* g) {
    TRLX_REQUIRE(g, TRLX_ERR_ARG, "t5 grouped d256 decode attention geometry: NULL result");
    *g = TrlxT5DecodeAttnGroupD256Geometry{};
    TRLX_REQUIRE(S >= 1 && S <= 0x7fffffffLL / 128, TRLX_ERR_ARG, "t5 grouped d256 decode attention geometry: S %lld", (long long)S);
    TRLX_REQUIRE(splits >= 1 && splits <= kGdMaxSplits, TRLX_ERR_ARG,
                 "t5 grouped d256 decode attention geometry: splits %lld (1 to %d)", (long long)splits, kGdMaxSplits);
    g->waves = kGdWaves;
    g->block_keys = kGdKeys;
    g->tile = kGdQ;
    t5_gd_ranges(S, splits, &g->cb, &g->ranges);
    g->max_splits = kGdMaxSplits;
    return TRLX_OK;
}

// The default `splits`: a pure function of the shape, not of live, the device or the strides.  Set
// from profiles/t5_cross_group_d256_bench.json ("Grouped decode cross-attention at d_kv
// 256"): a split above 1 only where the table shows it faster than splits 1 by more than the spread
// of the splits 1 samples.  W = the unsplit grid, nblk = the 32-key blocks.  nH 16, medians in us:
//   W 128, nblk 64 (P 8 x G 16, S 2048)   2   73.4 (69.3-76.8) at 1, 59.2 at 2, 64.9 at 4, 85.2 at 8
//   W 128, nblk 16 (P 8 x G 16, P 2 x G 64, P 8 x G 1; S 512, plain and padded)   1   2 is 0.2 to 3.6 us
//                  below 1 and inside 1's spread every time; 4 and 8 lose
//   W 16, nblk 16 (P 1 x G 8)             1   18 to 20 us at 2, 4, 8 against 22 to 24, 1's spread 16 to 23
//   W >= 256 (P 16 x G 8, P 32 x G 4, P 128 x G 1)   1   every split loses
// Grids below 128 workgroups at nblk >= 64 were not measured; they under-fill the chip more than
// the measured one and take its 2.
extern "C" int trlx_t5_decode_attn_group_d256_plan(int64_t P, int64_t G, int64_t n_heads, int64_t S) {
    if (P < 1 || G < 1 || n_heads < 1 || S < 1) return 1;
    if (P > 128 || n_heads > 128 || G > 128 * kGdQ) return 1;
    const int64_t W = P * n_heads * ((G + kGdQ - 1) / kGdQ), nblk = (S + kGdKeys - 1) / kGdKeys;
    return W <= 128 && nblk >= 64 ? 2 : 1;
}

extern "C" int trlx_t5_decode_attn_group_d256(const TrlxT5DecodeAttnGroupArgs* a, int64_t splits, void* workspace,
                                              int64_t workspace_bytes, void* stream) {
    const char* who = "t5 grouped d256 decode attention";
    T5GroupChecked c;   // the grid is (P * heads, ceil(G / 16), ranges); the merge's is rows * heads * 32 threads
    const int rc0 = t5_group_check(a, who, false, true, kGdQ, &c, kGdD);
    if (rc0) return rc0;
    TRLX_REQUIRE(splits >= 1 && splits <= kGdMaxSplits, TRLX_ERR_ARG, "%s: splits %lld (1 to %d)", who, (long long)splits,
                 kGdMaxSplits);
    int64_t cb, ranges;
    t5_gd_ranges(a->S, splits, &cb, &ranges);
    if (splits > 1) {
        const int64_t need = trlx_t5_decode_attn_group_d256_workspace_bytes(a->P * a->G, a->n_heads, a->S, splits);
        TRLX_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 && workspace_bytes >= need, TRLX_ERR_ARG,
                     "%s: workspace %p of %lld bytes (16-byte aligned, at least %lld bytes for %lld splits)", who, workspace,
                     (long long)workspace_bytes, (long long)need, (long long)splits);
    }
    T5GdArgs k = {};
    k.q = static_cast<const uint16_t*>(a->q);
    k.k = static_cast<const uint16_t*>(a->k);
    k.v = static_cast<const uint16_t*>(a->v);
    k.mask = a->key_mask;
    k.live = a->live;
    k.out = static_cast<uint16_t*>(a->out);
    k.ws = static_cast<float*>(workspace);
    k.ldq = c.ldq;
    k.k_sp = c.st[0], k.k_sh = c.st[1], k.k_ss = c.st[2];
    k.v_sp = c.st[3], k.v_sh = c.st[4], k.v_ss = c.st[5];
    k.nH = int(a->n_heads);
    k.G = int(a->G);
    k.S = int(a->S);
    k.cb = int(cb);
    k.ranges = int(ranges);
    k.rows = int(a->P * a->G);
    const bool masked = a->key_mask != nullptr, live = a->live != nullptr;
    if (splits == 1) {   // one launch, no workspace
        hipLaunchKernelGGL(t5_gd_pick<false>(masked, live), dim3(unsigned(a->P * a->n_heads), unsigned(c.tiles)),
                           dim3(kGdThreads), 0, (hipStream_t)stream, k);
        return check_launch("k_t5_decode_attn_group_d256");
    }
    hipLaunchKernelGGL(t5_gd_pick<true>(masked, live), dim3(unsigned(a->P * a->n_heads), unsigned(c.tiles), unsigned(ranges)),
                       dim3(kGdThreads), 0, (hipStream_t)stream, k);
    const int rc = check_launch("k_t5_decode_attn_group_d256");
    if (rc != TRLX_OK) return rc;
    const int64_t threads = a->P * a->G * a->n_heads * (kGdD / 8);
    hipLaunchKernelGGL(live ? k_t5_decode_attn_group_d256_merge<true> : k_t5_decode_attn_group_d256_merge<false>,
                       dim3(unsigned((threads + kGdThreads - 1) / kGdThreads)), dim3(kGdThreads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn_group_d256_merge");
}
