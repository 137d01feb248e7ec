// The decode-step projection of t5_decode_linear.hip with the rows spread over workgroups and a
// skip of the rows that have finished:
//   out = epilogue( prologue(x) . W^T )          x [M, K], W [N, K] (nn.Linear.weight), out [M, N]
// The same expression, forms and per-tile arithmetic as k_t5_decode_linear; what differs is which
// rows a workgroup takes.
//
// Grid (N / 16, ceil(M / RB)).  Workgroup (bx, by) owns output columns 16 bx .. and ONE block of at
// most RB = kDrRB rows, held as RB / 16 row tiles in one pass.  K is never split across workgroups:
// no atomics, no workspace.  A block's weight slab (16 rows of K, both slabs when gated) is read once
// per row block -- ceil(M / RB) times from L2 over the grid instead of once -- and the grid has
// ceil(M / RB) times the workgroups of k_t5_decode_linear's, which is the point at M 256.
//
// Rows of a block.  Without `live`, block by is rows [RB by, min(M, RB by + RB)).  With `live` (int64
// [M], nonzero = live) it is the live rows of rank [RB by, RB by + RB) in row order: every workgroup
// counts the live rows in front of each row itself -- the 256 threads take 256 rows a turn, a wave
// ballots, the four wave counts are added in wave order from LDS -- and keeps in LDS the original
// index of the rows whose rank falls into its range.  The grid does not depend on the live count (the
// host does not know it): a workgroup whose range is empty loads no weight.
// A dead row behaves as a zero input row and nothing of x is read for it: zeros out in the plain,
// norm and activation forms, out[m] = residual[m] in the residual form, and nothing at all when out
// is the residual (in place).  Workgroup (bx, by) writes the dead rows among the ORIGINAL rows
// [RB by, RB by + RB) for its 16 columns, so every element of out is written once per call or, for an
// in-place dead row, not at all.  No address into x is formed from a dead row: the row list holds live
// rows only and a lane past its end is clamped to the last of them.
//
// Per tile the arithmetic is k_t5_decode_linear's, restated here (that file is left as it is):
// 32-element chunk c belongs to wave (c / kDrKU) % 4, the four partials of a tile are added
// ((p0 + p1) + p2) + p3 by the tile's owner wave from LDS, rstd of a row is k_t5_rmsnorm_fwd's sum for
// D = K in the form chosen by K, one rounding per output.  None of it depends on the tile, pass or
// workgroup a row lands in, so a live row's output has the bits trlx_t5_decode_linear gives it.
#include "common.h"
#include "t5_row_math.h"

#ifndef TRLX_DR_ROWS_PER_BLOCK
#define TRLX_DR_ROWS_PER_BLOCK 32
#endif

namespace trlx {

typedef __bf16 dr_bf16x8 __attribute__((ext_vector_type(8)));
typedef float dr_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t dr_vec2u __attribute__((ext_vector_type(2)));

constexpr int kDrThreads = 256;
constexpr int kDrWaves = kDrThreads / kWave;
constexpr int kDrBN = 16;                 // output columns per workgroup
constexpr int kDrBM = 16;                 // rows per tile
constexpr int kDrBK = 32;                 // K per MFMA
constexpr int kDrKU = 4;                  // consecutive chunks a wave takes per turn
constexpr int kDrMaxTiles = 16;           // accumulator tiles (row tiles x slabs) of a wave
constexpr int kDrRB = TRLX_DR_ROWS_PER_BLOCK;   // rows per workgroup
constexpr int kDrMT = kDrRB / kDrBM;      // row tiles per workgroup
constexpr int kDrNormMaxK = 8192;         // t5_rmsnorm's limit
constexpr int kDrWaveRowMaxK = 1024;      // up to here the norm's sum takes one wave per row
constexpr int kDrMaxK = 16384;
// The largest M taken with live.  The scan would run for any M; the limit bounds what every workgroup
// re-reads from L2 (M live words: 32 KB here), a cost measured only at M 256.
constexpr int kDrMaxMLive = 4096;
constexpr int64_t kDrMaxRowBlocks = 65535;               // the grid's second dimension
static_assert(kDrRB % kDrBM == 0 && kDrRB >= kDrBM && 2 * kDrMT <= kDrMaxTiles, "the gated form keeps 2 RB / 16 tiles");

enum { kDrPlain = 0, kDrResidual = 1, kDrAct = 2 };

struct DrArgs {
    const uint16_t *x, *w, *nw, *res;
    uint16_t* out;
    const int64_t* live;
    int64_t ld_x, ld_w, ld_res, ld_out;
    int M, K, N;     // N: output columns (F of the activation forms)
    float eps;
};

__device__ __forceinline__ vec4u dr_ld16(const uint16_t* p) { return *reinterpret_cast<const vec4u*>(p); }

// s continues a thread's sum of squares over one more unit, in element order
__device__ __forceinline__ float dr_sumsq_unit(float s, const uint16_t* p) {
    float f[8];
    BF16T::unpack(dr_ld16(p), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) s += f[i] * f[i];
    return s;
}

template <int NB, int EPI, int ACT, bool NORM>
__global__ __launch_bounds__(kDrThreads) void k_t5_decode_linear_rows(DrArgs a) {
    constexpr int MT = kDrMT;
    static_assert(MT * NB <= kDrMaxTiles && (NB == 1 || EPI == kDrAct), "tile budget");
    __shared__ dr_f32x4 part[MT * NB * (kDrWaves - 1) * kWave];   // [tile][wave slot][lane]
    __shared__ float s_rstd[NORM ? kDrRB : 1];
    __shared__ float s_red[2 * kDrWaves];
    __shared__ int s_row[kDrRB];                                  // the block's rows, original indices
    __shared__ int s_cnt[2 * kDrWaves];
    const int tid = int(threadIdx.x), lane = tid & (kWave - 1), wave = tid / kWave;
    const int fr = lane & 15, fc = lane >> 4;
    const int n0 = int(blockIdx.x) * kDrBN;
    const int first = int(blockIdx.y) * kDrRB;   // the block's first original row and its first live rank
    const int nchunk = a.K / kDrBK;

    int rows;
    if (a.live) {
        // rank of a live row = live rows in front of it: 256 rows a turn, ballot, wave counts in wave order
        int seen = 0, turn = 0;
#pragma unroll 1
        for (int base = 0; base < a.M && seen < first + kDrRB; base += kDrThreads) {
            const int r = base + tid;
            const bool on = r < a.M && a.live[r] != 0;
            const unsigned long long votes = __ballot(on);
            int* cnt = s_cnt + turn * kDrWaves;                    // two sets in turn: one barrier per turn
            turn ^= 1;
            if (lane == 0) cnt[wave] = __popcll(votes);
            __syncthreads();
            int before = seen;
#pragma unroll
            for (int w = 0; w < kDrWaves; ++w) {
                if (w < wave) before += cnt[w];
                seen += cnt[w];
            }
            const int rank = before + __popcll(votes & ((1ull << lane) - 1ull)) - first;
            if (on && rank >= 0 && rank < kDrRB) s_row[rank] = r;
        }
        rows = seen - first < kDrRB ? seen - first : kDrRB;
        // the dead rows among the original rows of this block, these 16 columns
        if (EPI != kDrResidual || a.res != a.out) {
#pragma unroll 1
            for (int i = tid; i < kDrRB * (kDrBN / 4); i += kDrThreads) {
                const int64_t m = first + i / (kDrBN / 4);
                const int n = n0 + (i % (kDrBN / 4)) * 4;
                if (m >= a.M || a.live[m] != 0) continue;
                dr_vec2u o = {0u, 0u};
                if constexpr (EPI == kDrResidual) o = *reinterpret_cast<const dr_vec2u*>(a.res + m * a.ld_res + n);
                *reinterpret_cast<dr_vec2u*>(a.out + m * a.ld_out + n) = o;
            }
        }
    } else {
        rows = a.M - first < kDrRB ? a.M - first : kDrRB;
        if (tid < rows) s_row[tid] = first + tid;
    }
    if (rows <= 0) return;                                         // workgroup-uniform: no live row of this rank range
    __syncthreads();

    const uint16_t* wrow[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) wrow[s] = a.w + (int64_t(s) * a.N + n0 + fr) * a.ld_w + fc * 8;

    if constexpr (NORM) {
        if (a.K <= kDrWaveRowMaxK) {
#pragma unroll 1
            for (int r = wave; r < rows; r += kDrWaves) {
                const uint16_t* xr = a.x + int64_t(s_row[r]) * a.ld_x;
                float s = 0.f;
                for (int c = lane * 8; c < a.K; c += kWave * 8) s = dr_sumsq_unit(s, xr + c);
                s = wave_sum(s);
                if (lane == 0) s_rstd[r] = rn_rstd(s, a.K, a.eps);
            }
        } else {
            int turn = 0;
#pragma unroll 1
            for (int r = 0; r < rows; ++r) {
                const uint16_t* xr = a.x + int64_t(s_row[r]) * a.ld_x;
                float s = 0.f;
                for (int c = tid * 8; c < a.K; c += kDrThreads * 8) s = dr_sumsq_unit(s, xr + c);
                s = wave_sum(s);
                float* sl = s_red + turn * kDrWaves;               // two sets in turn: one barrier per sum
                turn ^= 1;
                if (lane == 0) sl[wave] = s;
                __syncthreads();
                if (tid == 0) s_rstd[r] = rn_rstd(((sl[0] + sl[1]) + sl[2]) + sl[3], a.K, a.eps);
            }
        }
        __syncthreads();
    }

    // this lane's token row of every tile, clamped to the block's last row (its results are dropped)
    const uint16_t* xrow[MT];
    float rs[NORM ? MT : 1];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int lr = mt * kDrBM + fr < rows ? mt * kDrBM + fr : rows - 1;
        xrow[mt] = a.x + int64_t(s_row[lr]) * a.ld_x + fc * 8;
        if constexpr (NORM) rs[mt] = s_rstd[lr];
    }
    dr_f32x4 acc[MT][NB];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int s = 0; s < NB; ++s) acc[mt][s] = dr_f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int c0 = wave * kDrKU; c0 < nchunk; c0 += kDrWaves * kDrKU) {
        vec4u wf[NB][kDrKU], nwf[NORM ? kDrKU : 1];
#pragma unroll
        for (int u = 0; u < kDrKU; ++u) {
            const int c = c0 + u < nchunk ? c0 + u : nchunk - 1;   // clamped: loaded, not used
#pragma unroll
            for (int s = 0; s < NB; ++s) wf[s][u] = dr_ld16(wrow[s] + c * kDrBK);
            if constexpr (NORM) nwf[u] = dr_ld16(a.nw + c * kDrBK + fc * 8);
        }
#pragma unroll
        for (int u = 0; u < kDrKU; ++u) {
            if (c0 + u >= nchunk) break;                           // wave-uniform
            float g[NORM ? 8 : 1];
            if constexpr (NORM) BF16T::unpack(nwf[u], g);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                vec4u xv = dr_ld16(xrow[mt] + (c0 + u) * kDrBK);
                if constexpr (NORM) {
                    float f[8];
                    BF16T::unpack(xv, f);
#pragma unroll
                    for (int i = 0; i < 8; ++i) f[i] = g[i] * (f[i] * rs[mt]);
                    xv = BF16T::pack(f);
                }
#pragma unroll
                for (int s = 0; s < NB; ++s)
                    acc[mt][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dr_bf16x8, wf[s][u]),
                                                                         __builtin_bit_cast(dr_bf16x8, xv), acc[mt][s], 0, 0, 0);
            }
        }
    }

    // the partial sums of a tile go to its owner wave, which adds the four in wave order
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int owner = mt % kDrWaves;
        if (wave != owner) {
            const int slot = wave < owner ? wave : wave - 1;
#pragma unroll
            for (int s = 0; s < NB; ++s) part[((mt * NB + s) * (kDrWaves - 1) + slot) * kWave + lane] = acc[mt][s];
        }
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int owner = mt % kDrWaves;
        if (wave != owner) continue;
        dr_f32x4 sum[NB];
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            dr_f32x4 t = dr_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < kDrWaves; ++w) {
                const int slot = w < owner ? w : w - 1;
                const dr_f32x4 p = w == owner ? acc[mt][s] : part[((mt * NB + s) * (kDrWaves - 1) + slot) * kWave + lane];
                t = w == 0 ? p : t + p;
            }
            sum[s] = t;
        }
        const int lr = mt * kDrBM + fr;
        if (lr >= rows) continue;
        const int64_t m = s_row[lr];
        const int n = n0 + fc * 4;
        float y[4];
        if constexpr (EPI == kDrResidual) {
            const dr_vec2u rv = *reinterpret_cast<const dr_vec2u*>(a.res + m * a.ld_res + n);
            y[0] = sum[0][0] + bf_lo(rv.x), y[1] = sum[0][1] + bf_hi(rv.x);
            y[2] = sum[0][2] + bf_lo(rv.y), y[3] = sum[0][3] + bf_hi(rv.y);
        } else if constexpr (EPI == kDrAct) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float act, d;
                fa_eval<ACT, false>(sum[0][q], act, d);
                y[q] = NB == 2 ? act * sum[NB - 1][q] : act;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) y[q] = sum[0][q];
        }
        dr_vec2u o;
        o.x = pack_bf2(y[0], y[1]), o.y = pack_bf2(y[2], y[3]);
        *reinterpret_cast<dr_vec2u*>(a.out + m * a.ld_out + n) = o;
    }
}

typedef void (*dr_kernel_t)(DrArgs);

template <int NB, int EPI, int ACT>
static dr_kernel_t dr_pick_norm(bool norm) {
    return norm ? k_t5_decode_linear_rows<NB, EPI, ACT, true> : k_t5_decode_linear_rows<NB, EPI, ACT, false>;
}

template <int NB>
static dr_kernel_t dr_pick_act(int act, bool norm) {
    switch (act) {
        case TRLX_T5_ACT_RELU: return dr_pick_norm<NB, kDrAct, TRLX_T5_ACT_RELU>(norm);
        case TRLX_T5_ACT_GELU_NEW: return dr_pick_norm<NB, kDrAct, TRLX_T5_ACT_GELU_NEW>(norm);
        default: return dr_pick_norm<NB, kDrAct, TRLX_T5_ACT_SILU>(norm);
    }
}

// One operand as a byte range.
struct DrOp {
    const char* name;
    uintptr_t lo, hi;
};

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_decode_linear_rows_geometry(TrlxT5DecodeLinearRowsGeometry* g) {
    TRLX_REQUIRE(g, TRLX_ERR_ARG, "t5 decode linear rows geometry: NULL geometry");
    g->threads = kDrThreads;
    g->cols_per_block = kDrBN;
    g->rows_per_tile = kDrBM;
    g->rows_per_block = kDrRB;
    g->max_m_live = kDrMaxMLive;
    g->reserved = 0;
    return TRLX_OK;
}

extern "C" int trlx_t5_decode_linear_rows(const trlx_t5_decode_linear_rows_args* a, void* stream) {
    const char* who = "t5 decode linear rows";
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->x && a->weight && a->out, TRLX_ERR_ARG, "%s: NULL x / weight / out", who);
    TRLX_REQUIRE(a->dtype == TRLX_BF16, TRLX_ERR_DTYPE, "%s: dtype %d (bfloat16 only)", who, a->dtype);
    const bool has_act = a->act != TRLX_T5_ACT_NONE, gated = a->gated != 0, norm = a->norm_weight != nullptr;
    TRLX_REQUIRE(!has_act || a->act == TRLX_T5_ACT_RELU || a->act == TRLX_T5_ACT_GELU_NEW || a->act == TRLX_T5_ACT_SILU,
                 TRLX_ERR_ARG, "%s: activation %d (none -1, relu 0, gelu_new 1, silu 2)", who, a->act);
    TRLX_REQUIRE(!gated || has_act, TRLX_ERR_ARG, "%s: gated without an activation", who);
    TRLX_REQUIRE(!(has_act && a->residual), TRLX_ERR_ARG, "%s: a residual and an activation (one epilogue at most)", who);
    TRLX_REQUIRE(a->M >= 1 && a->M <= 0x7fffffffLL, TRLX_ERR_SHAPE, "%s: M %lld (1 to 2^31 - 1)", who, (long long)a->M);
    TRLX_REQUIRE(a->M <= kDrMaxRowBlocks * kDrRB, TRLX_ERR_SHAPE, "%s: M %lld (at most %lld row blocks of %d rows)", who,
                 (long long)a->M, (long long)kDrMaxRowBlocks, kDrRB);
    TRLX_REQUIRE(!a->live || a->M <= kDrMaxMLive, TRLX_ERR_SHAPE, "%s: M %lld with live rows (at most %d: every workgroup reads all M live words)",
                 who, (long long)a->M, kDrMaxMLive);
    TRLX_REQUIRE(a->K >= kDrBK && a->K % kDrBK == 0 && a->K <= kDrMaxK, TRLX_ERR_SHAPE,
                 "%s: K %lld (a multiple of %d, %d to %d)", who, (long long)a->K, kDrBK, kDrBK, kDrMaxK);
    TRLX_REQUIRE(!norm || a->K <= kDrNormMaxK, TRLX_ERR_SHAPE, "%s: K %lld with a norm weight (at most %d, t5_rmsnorm's limit)",
                 who, (long long)a->K, kDrNormMaxK);
    TRLX_REQUIRE(a->N >= kDrBN && a->N % kDrBN == 0 && a->N <= (int64_t(1) << 30), TRLX_ERR_SHAPE,
                 "%s: N %lld (output columns: a multiple of %d, %d to 2^30)", who, (long long)a->N, kDrBN, kDrBN);
    TRLX_REQUIRE(!norm || a->eps == a->eps, TRLX_ERR_ARG, "%s: eps is NaN", who);
    const int nb = gated ? 2 : 1;
    const int64_t wrows = a->N * nb;
    struct {
        const char* name;
        const void* p;
        int64_t ld, rows, cols;
    } in[5] = {{"x", a->x, a->ld_x, a->M, a->K},
               {"weight", a->weight, a->ld_w, wrows, a->K},
               {"out", a->out, a->ld_out, a->M, a->N},
               {"residual", a->residual, a->ld_residual, a->M, a->N},
               {"norm_weight", a->norm_weight, a->K, 1, a->K}};
    DrOp ops[5];
    for (int i = 0; i < 5; ++i) {
        ops[i] = {in[i].name, 0, 0};
        if (!in[i].p) continue;
        const uintptr_t p = reinterpret_cast<uintptr_t>(in[i].p);
        TRLX_REQUIRE(p % 16 == 0, TRLX_ERR_ARG, "%s: %s not aligned to 16 bytes", who, in[i].name);
        TRLX_REQUIRE(in[i].ld >= in[i].cols, TRLX_ERR_STRIDE, "%s: %s row stride %lld below its %lld columns", who, in[i].name,
                     (long long)in[i].ld, (long long)in[i].cols);
        TRLX_REQUIRE(in[i].ld % 8 == 0, TRLX_ERR_STRIDE, "%s: %s row stride %lld off the 16-byte grid", who, in[i].name,
                     (long long)in[i].ld);
        int64_t span;
        TRLX_REQUIRE(!__builtin_mul_overflow(in[i].rows - 1, in[i].ld, &span) && span <= (int64_t(1) << 59), TRLX_ERR_STRIDE,
                     "%s: %s rows %lld apart do not fit the address space", who, in[i].name, (long long)in[i].ld);
        ops[i].lo = p, ops[i].hi = p + uintptr_t((span + in[i].cols) * 2);
    }
    // out shares no byte range with x, weight or norm_weight; with residual only as the very same rows
    const DrOp& out = ops[2];
    for (int i = 0; i < 5; ++i) {
        if (i == 2 || !in[i].p || out.hi <= ops[i].lo || ops[i].hi <= out.lo) continue;
        const bool same_rows = i == 3 && a->residual == a->out && a->ld_residual == a->ld_out;
        TRLX_REQUIRE(same_rows, TRLX_ERR_ARG, "%s: out overlaps %s%s", who, in[i].name,
                     i == 3 ? " (taken only as the very same rows: same pointer, same stride)" : "");
    }
    if (a->live) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(a->live), hi = lo + uintptr_t(a->M) * 8;
        TRLX_REQUIRE(lo % 8 == 0, TRLX_ERR_ARG, "%s: live not aligned to 8 bytes", who);
        TRLX_REQUIRE(out.hi <= lo || hi <= out.lo, TRLX_ERR_ARG, "%s: out overlaps live", who);
    }
    DrArgs k = {};
    k.x = static_cast<const uint16_t*>(a->x), k.w = static_cast<const uint16_t*>(a->weight);
    k.nw = static_cast<const uint16_t*>(a->norm_weight), k.res = static_cast<const uint16_t*>(a->residual);
    k.out = static_cast<uint16_t*>(a->out), k.live = a->live;
    k.ld_x = a->ld_x, k.ld_w = a->ld_w, k.ld_res = a->ld_residual, k.ld_out = a->ld_out;
    k.M = int(a->M), k.K = int(a->K), k.N = int(a->N), k.eps = a->eps;
    dr_kernel_t fn;
    if (has_act)
        fn = gated ? dr_pick_act<2>(a->act, norm) : dr_pick_act<1>(a->act, norm);
    else if (a->residual)
        fn = dr_pick_norm<1, kDrResidual, TRLX_T5_ACT_RELU>(norm);
    else
        fn = dr_pick_norm<1, kDrPlain, TRLX_T5_ACT_RELU>(norm);
    const unsigned row_blocks = unsigned((a->M + kDrRB - 1) / kDrRB);
    hipLaunchKernelGGL(fn, dim3(unsigned(a->N / kDrBN), row_blocks), dim3(kDrThreads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_linear_rows");
}
