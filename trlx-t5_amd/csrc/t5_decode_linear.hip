// A decode-step projection with its neighbours folded in, one launch:
//   out = epilogue( prologue(x) . W^T )          x [M, K], W [N, K] (nn.Linear.weight), out [M, N]
//   prologue   none, or T5's RMSNorm: xh[m, k] = bf16(nw[k] * (x[m, k] * rstd[m]))
//   epilogue   none, out = bf16(acc + residual), or out = bf16(act(u) [* v]) with u, v the
//              accumulators of rows j and F + j of a packed [2F, K] weight
// bf16 on v_mfma_f32_16x16x32_bf16, fp32 accumulation.  Built for M <= 256 rows and weights of a few
// MB, where a layer's time is its launch count: the norm in front, the residual add behind and the
// gated activation behind `wi` ride in the projection's launch and their bf16 round trips through
// HBM (the normed rows, u | v, the projection output before the add) go away.
//
// Blocking.  A workgroup is 4 waves and owns kDlBN = 16 output columns (both weight slabs of them
// when gated); it walks the rows in passes of MT 16-row tiles, MT in {1, 4, 8, 16} by M.  K is never
// split across workgroups: no atomics, no workspace.  Inside the workgroup K is split across the
// waves -- 32-element chunk c belongs to wave (c / kDlKU) % 4, so a wave reads kDlKU * 64 B = 256 B
// of a weight row at a time with kDlKU weight fragments in flight -- and the four partial
// accumulators of a tile are added in wave order ((p0 + p1) + p2) + p3 by the tile's owner wave
// (tile mt belongs to wave mt % 4) from LDS: a fixed order, two runs give the same bits.  A wave
// holds its weight fragments of a chunk in registers over all MT row tiles, so a pass reads each
// weight byte once; x comes from L2 (every workgroup reads all of it).
//
// The MFMA takes the weight fragment as its first operand: D[i][j] with i the weight row and j the
// token, so lane (fr, fc) = (lane & 15, lane >> 4) ends with output columns n0 + 4 fc .. + 3 of row
// fr -- one 8-byte store, one 8-byte residual load.
//
// Prologue.  rstd of a row runs the very sum of k_t5_rmsnorm_fwd for D = K (t5_rmsnorm.hip): the row
// form by K (one wave per row up to 1024, the workgroup per row above), element j in unit j / 8, unit
// u in thread u % TEAM at step u / TEAM, a thread's squares added in element order, the xor
// butterfly, the four waves in order, rn_rstd.  With the product nw * (x * rstd) and its one rounding,
// xh has the bits of t5_rmsnorm(x, nw).  Two passes over the L2-resident rows: the sums first (rstd
// of the pass's rows in LDS), the product as the fragments are loaded.  The normed rows are never
// written.
#include "common.h"
#include "t5_row_math.h"

namespace trlx {

typedef __bf16 dl_bf16x8 __attribute__((ext_vector_type(8)));
typedef float dl_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t dl_vec2u __attribute__((ext_vector_type(2)));

constexpr int kDlThreads = 256;
constexpr int kDlWaves = kDlThreads / kWave;
constexpr int kDlBN = 16;                 // output columns per workgroup
constexpr int kDlBM = 16;                 // rows per tile
constexpr int kDlBK = 32;                 // K per MFMA
constexpr int kDlKU = 4;                  // consecutive chunks a wave takes per turn
constexpr int kDlMaxTiles = 16;           // accumulator tiles (row tiles x slabs) of a wave
constexpr int kDlNormMaxK = 8192;         // t5_rmsnorm's limit
constexpr int kDlWaveRowMaxK = 1024;      // up to here the norm's sum takes one wave per row
constexpr int kDlMaxK = 16384;

enum { kDlPlain = 0, kDlResidual = 1, kDlAct = 2 };

struct DlArgs {
    const uint16_t *x, *w, *nw, *res;
    uint16_t* out;
    int64_t ld_x, ld_w, ld_res, ld_out, M;
    int K, N;        // N: output columns (F of the activation forms)
    float eps;
};

__device__ __forceinline__ vec4u dl_ld16(const uint16_t* p) { return *reinterpret_cast<const vec4u*>(p); }

// s continues a thread's sum of squares over one more unit, in element order
__device__ __forceinline__ float dl_sumsq_unit(float s, const uint16_t* p) {
    float f[8];
    BF16T::unpack(dl_ld16(p), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) s += f[i] * f[i];
    return s;
}

template <int MT, int NB, int EPI, int ACT, bool NORM>
__global__ __launch_bounds__(kDlThreads) void k_t5_decode_linear(DlArgs a) {
    static_assert(MT * NB <= kDlMaxTiles && (NB == 1 || EPI == kDlAct), "tile budget");
    __shared__ dl_f32x4 part[MT * NB * (kDlWaves - 1) * kWave];   // [tile][wave slot][lane]
    __shared__ float s_rstd[NORM ? MT * kDlBM : 1];
    __shared__ float s_red[2 * kDlWaves];
    const int tid = int(threadIdx.x), lane = tid & (kWave - 1), wave = tid / kWave;
    const int fr = lane & 15, fc = lane >> 4;
    const int n0 = int(blockIdx.x) * kDlBN;
    const int nchunk = a.K / kDlBK;
    const uint16_t* wrow[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) wrow[s] = a.w + (int64_t(s) * a.N + n0 + fr) * a.ld_w + fc * 8;

#pragma unroll 1
    for (int64_t m0 = 0; m0 < a.M; m0 += MT * kDlBM) {
        const int rows = int(a.M - m0 < MT * kDlBM ? a.M - m0 : MT * kDlBM);
        __syncthreads();                                           // the pass before is done with part and s_rstd
        if constexpr (NORM) {
            if (a.K <= kDlWaveRowMaxK) {
#pragma unroll 1
                for (int r = wave; r < rows; r += kDlWaves) {
                    const uint16_t* xr = a.x + (m0 + r) * a.ld_x;
                    float s = 0.f;
                    for (int c = lane * 8; c < a.K; c += kWave * 8) s = dl_sumsq_unit(s, xr + c);
                    s = wave_sum(s);
                    if (lane == 0) s_rstd[r] = rn_rstd(s, a.K, a.eps);
                }
            } else {
                int turn = 0;
#pragma unroll 1
                for (int r = 0; r < rows; ++r) {
                    const uint16_t* xr = a.x + (m0 + r) * a.ld_x;
                    float s = 0.f;
                    for (int c = tid * 8; c < a.K; c += kDlThreads * 8) s = dl_sumsq_unit(s, xr + c);
                    s = wave_sum(s);
                    float* sl = s_red + turn * kDlWaves;           // two sets in turn: one barrier per sum
                    turn ^= 1;
                    if (lane == 0) sl[wave] = s;
                    __syncthreads();
                    if (tid == 0) s_rstd[r] = rn_rstd(((sl[0] + sl[1]) + sl[2]) + sl[3], a.K, a.eps);
                }
            }
            __syncthreads();
        }

        // this lane's token row of every tile, clamped to the pass's last row (its results are dropped)
        const uint16_t* xrow[MT];
        float rs[NORM ? MT : 1];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int lr = mt * kDlBM + fr < rows ? mt * kDlBM + fr : rows - 1;
            xrow[mt] = a.x + (m0 + lr) * a.ld_x + fc * 8;
            if constexpr (NORM) rs[mt] = s_rstd[lr];
        }
        dl_f32x4 acc[MT][NB];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int s = 0; s < NB; ++s) acc[mt][s] = dl_f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
        for (int c0 = wave * kDlKU; c0 < nchunk; c0 += kDlWaves * kDlKU) {
            vec4u wf[NB][kDlKU], nwf[NORM ? kDlKU : 1];
#pragma unroll
            for (int u = 0; u < kDlKU; ++u) {
                const int c = c0 + u < nchunk ? c0 + u : nchunk - 1;   // clamped: loaded, not used
#pragma unroll
                for (int s = 0; s < NB; ++s) wf[s][u] = dl_ld16(wrow[s] + c * kDlBK);
                if constexpr (NORM) nwf[u] = dl_ld16(a.nw + c * kDlBK + fc * 8);
            }
#pragma unroll
            for (int u = 0; u < kDlKU; ++u) {
                if (c0 + u >= nchunk) break;                       // wave-uniform
                float g[NORM ? 8 : 1];
                if constexpr (NORM) BF16T::unpack(nwf[u], g);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    vec4u xv = dl_ld16(xrow[mt] + (c0 + u) * kDlBK);
                    if constexpr (NORM) {
                        float f[8];
                        BF16T::unpack(xv, f);
#pragma unroll
                        for (int i = 0; i < 8; ++i) f[i] = g[i] * (f[i] * rs[mt]);
                        xv = BF16T::pack(f);
                    }
#pragma unroll
                    for (int s = 0; s < NB; ++s)
                        acc[mt][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dl_bf16x8, wf[s][u]),
                                                                             __builtin_bit_cast(dl_bf16x8, xv), acc[mt][s], 0, 0, 0);
                }
            }
        }

        // the partial sums of a tile go to its owner wave, which adds the four in wave order
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int owner = mt % kDlWaves;
            if (wave != owner) {
                const int slot = wave < owner ? wave : wave - 1;
#pragma unroll
                for (int s = 0; s < NB; ++s) part[((mt * NB + s) * (kDlWaves - 1) + slot) * kWave + lane] = acc[mt][s];
            }
        }
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int owner = mt % kDlWaves;
            if (wave != owner) continue;
            dl_f32x4 sum[NB];
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                dl_f32x4 t = dl_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int w = 0; w < kDlWaves; ++w) {
                    const int slot = w < owner ? w : w - 1;
                    const dl_f32x4 p = w == owner ? acc[mt][s] : part[((mt * NB + s) * (kDlWaves - 1) + slot) * kWave + lane];
                    t = w == 0 ? p : t + p;
                }
                sum[s] = t;
            }
            const int lr = mt * kDlBM + fr;
            if (lr >= rows) continue;
            const int64_t m = m0 + lr;
            const int n = n0 + fc * 4;
            float y[4];
            if constexpr (EPI == kDlResidual) {
                const dl_vec2u rv = *reinterpret_cast<const dl_vec2u*>(a.res + m * a.ld_res + n);
                y[0] = sum[0][0] + bf_lo(rv.x), y[1] = sum[0][1] + bf_hi(rv.x);
                y[2] = sum[0][2] + bf_lo(rv.y), y[3] = sum[0][3] + bf_hi(rv.y);
            } else if constexpr (EPI == kDlAct) {
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
            dl_vec2u o;
            o.x = pack_bf2(y[0], y[1]), o.y = pack_bf2(y[2], y[3]);
            *reinterpret_cast<dl_vec2u*>(a.out + m * a.ld_out + n) = o;
        }
    }
}

typedef void (*dl_kernel_t)(DlArgs);

template <int MT, int NB, int EPI, int ACT>
static dl_kernel_t dl_pick_norm(bool norm) {
    return norm ? k_t5_decode_linear<MT, NB, EPI, ACT, true> : k_t5_decode_linear<MT, NB, EPI, ACT, false>;
}

template <int NB, int EPI, int ACT>
static dl_kernel_t dl_pick_mt(int mt, bool norm) {
    switch (mt) {
        case 1: return dl_pick_norm<1, NB, EPI, ACT>(norm);
        case 4: return dl_pick_norm<4, NB, EPI, ACT>(norm);
        case 8: return dl_pick_norm<8, NB, EPI, ACT>(norm);
        default:
            if constexpr (NB == 1) return dl_pick_norm<16, NB, EPI, ACT>(norm);
            else return dl_pick_norm<8, NB, EPI, ACT>(norm);
    }
}

template <int NB>
static dl_kernel_t dl_pick_act(int act, int mt, bool norm) {
    switch (act) {
        case TRLX_T5_ACT_RELU: return dl_pick_mt<NB, kDlAct, TRLX_T5_ACT_RELU>(mt, norm);
        case TRLX_T5_ACT_GELU_NEW: return dl_pick_mt<NB, kDlAct, TRLX_T5_ACT_GELU_NEW>(mt, norm);
        default: return dl_pick_mt<NB, kDlAct, TRLX_T5_ACT_SILU>(mt, norm);
    }
}

// row tiles per pass for M rows and NB slabs
static int dl_row_tiles(int64_t M, int nb) {
    const int64_t tiles = (M + kDlBM - 1) / kDlBM;
    const int cap = kDlMaxTiles / nb;
    const int mt = tiles <= 1 ? 1 : tiles <= 4 ? 4 : tiles <= 8 ? 8 : 16;
    return mt < cap ? mt : cap;
}

// One operand as a byte range.
struct DlOp {
    const char* name;
    uintptr_t lo, hi;
};

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_decode_linear_geometry(TrlxT5DecodeLinearGeometry* g) {
    TRLX_REQUIRE(g, TRLX_ERR_ARG, "t5 decode linear geometry: NULL geometry");
    g->threads = kDlThreads;
    g->cols_per_block = kDlBN;
    g->rows_per_tile = kDlBM;
    g->k_per_chunk = kDlBK;
    g->chunks_per_wave_turn = kDlKU;
    g->max_row_tiles = kDlMaxTiles;
    g->max_k = kDlMaxK;
    g->norm_max_k = kDlNormMaxK;
    g->norm_wave_row_max_k = kDlWaveRowMaxK;
    g->reserved = 0;
    return TRLX_OK;
}

extern "C" int trlx_t5_decode_linear(const trlx_t5_decode_linear_args* a, void* stream) {
    const char* who = "t5 decode linear";
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->x && a->weight && a->out, TRLX_ERR_ARG, "%s: NULL x / weight / out", who);
    TRLX_REQUIRE(a->dtype == TRLX_BF16, TRLX_ERR_DTYPE, "%s: dtype %d (bfloat16 only)", who, a->dtype);
    const bool has_act = a->act != TRLX_T5_ACT_NONE, gated = a->gated != 0, norm = a->norm_weight != nullptr;
    TRLX_REQUIRE(!has_act || a->act == TRLX_T5_ACT_RELU || a->act == TRLX_T5_ACT_GELU_NEW || a->act == TRLX_T5_ACT_SILU,
                 TRLX_ERR_ARG, "%s: activation %d (none -1, relu 0, gelu_new 1, silu 2)", who, a->act);
    TRLX_REQUIRE(!gated || has_act, TRLX_ERR_ARG, "%s: gated without an activation", who);
    TRLX_REQUIRE(!(has_act && a->residual), TRLX_ERR_ARG, "%s: a residual and an activation (one epilogue at most)", who);
    TRLX_REQUIRE(a->M >= 1 && a->M <= 0x7fffffffLL, TRLX_ERR_SHAPE, "%s: M %lld (1 to 2^31 - 1)", who, (long long)a->M);
    TRLX_REQUIRE(a->K >= kDlBK && a->K % kDlBK == 0 && a->K <= kDlMaxK, TRLX_ERR_SHAPE,
                 "%s: K %lld (a multiple of %d, %d to %d)", who, (long long)a->K, kDlBK, kDlBK, kDlMaxK);
    TRLX_REQUIRE(!norm || a->K <= kDlNormMaxK, TRLX_ERR_SHAPE, "%s: K %lld with a norm weight (at most %d, t5_rmsnorm's limit)",
                 who, (long long)a->K, kDlNormMaxK);
    TRLX_REQUIRE(a->N >= kDlBN && a->N % kDlBN == 0 && a->N <= (int64_t(1) << 30), TRLX_ERR_SHAPE,
                 "%s: N %lld (output columns: a multiple of %d, %d to 2^30)", who, (long long)a->N, kDlBN, kDlBN);
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
    DlOp ops[5];
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
    const DlOp& out = ops[2];
    for (int i = 0; i < 5; ++i) {
        if (i == 2 || !in[i].p || out.hi <= ops[i].lo || ops[i].hi <= out.lo) continue;
        const bool same_rows = i == 3 && a->residual == a->out && a->ld_residual == a->ld_out;
        TRLX_REQUIRE(same_rows, TRLX_ERR_ARG, "%s: out overlaps %s%s", who, in[i].name,
                     i == 3 ? " (taken only as the very same rows: same pointer, same stride)" : "");
    }
    DlArgs k = {};
    k.x = static_cast<const uint16_t*>(a->x), k.w = static_cast<const uint16_t*>(a->weight);
    k.nw = static_cast<const uint16_t*>(a->norm_weight), k.res = static_cast<const uint16_t*>(a->residual);
    k.out = static_cast<uint16_t*>(a->out);
    k.ld_x = a->ld_x, k.ld_w = a->ld_w, k.ld_res = a->ld_residual, k.ld_out = a->ld_out, k.M = a->M;
    k.K = int(a->K), k.N = int(a->N), k.eps = a->eps;
    const int mt = dl_row_tiles(a->M, nb);
    dl_kernel_t fn;
    if (has_act)
        fn = gated ? dl_pick_act<2>(a->act, mt, norm) : dl_pick_act<1>(a->act, mt, norm);
    else if (a->residual)
        fn = dl_pick_mt<1, kDlResidual, TRLX_T5_ACT_RELU>(mt, norm);
    else
        fn = dl_pick_mt<1, kDlPlain, TRLX_T5_ACT_RELU>(mt, norm);
    hipLaunchKernelGGL(fn, dim3(unsigned(a->N / kDlBN)), dim3(kDlThreads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_linear");
}
