// T5 RMSNorm (HF T5LayerNorm: no mean subtraction, no bias, eps inside the root) with the residual
// add of the sub-layer before it, forward and backward:
//   forward   h = residual + x (rounded once, add form only)     rstd_n = 1 / sqrt(mean_j h[n,j]^2 + eps)
//             y[n,j] = w[j] * (h[n,j] * rstd_n)                   one launch, h and y written, x / residual read once
//   backward  g = w dy, hh = h rstd, c_n = mean_j g hh
//             dh = rstd (g - hh c) + dh_in,   dw[j] = sum_n dy[n,j] hh[n,j]
//             one row launch (dh, and per-workgroup fp32 partials of dw) and one finish launch; no atomics
// HBM-bound row work.  A workgroup is 4 waves.  Rows of D <= kRnWaveMaxD are taken by one wave each
// (4 rows per workgroup pass, the row reductions are wave shuffles, no barrier); wider rows by the
// whole workgroup (one row per pass, one barrier per reduction).  Either way a thread holds its E
// elements of the row in registers from the sum of squares to the stores -- E in {8, 16, 32}, the
// smallest that covers D -- so a row is read once; D above kRnMaxD = 256 * 32 is refused.  A
// workgroup walks the row blocks b = blockIdx, blockIdx + G, ... with G = min(row blocks,
// kRnMaxPartials); in the backward each thread keeps the dw sums of its own columns in registers over
// that walk, the 4 waves of a wave-per-row workgroup add theirs through LDS in wave order, and the
// workgroup stores row blockIdx of the [G, D] workspace: every element the finish kernel reads was
// written, so nothing is cleared.
//
// Element j of a row belongs to unit j / W (W = elements per 16 bytes), unit u to thread u % TEAM at
// step u / TEAM.  The vector form moves a unit in one 16-byte access; the element form (a pointer,
// a stride or D off the 16-byte grid) moves the same unit's elements one by one.  Both run the same
// fp32 operations in the same order on the same values, so they give the same bits.
#include <string.h>

#include <type_traits>

#include "common.h"
#include "t5_row_math.h"

namespace trlx {

constexpr int kRnThreads = 256;
constexpr int kRnMaxPartials = 1024;          // G's cap: 4 workgroups (16 waves) per CU
constexpr int kRnWaveMaxD = 1024;             // up to here one wave per row
constexpr int kRnMaxD = 8192;                 // 256 threads x 32 elements
constexpr int kRnBreaks[5] = {512, 1024, 2048, 4096, 8192};   // the largest D of each (TEAM, E) form
constexpr int kRnFinCols = 32;                // finish kernel: columns per workgroup ...
constexpr int kRnFinSlices = 32;              // ... and slices of G, one thread per (slice, column)
static_assert(kRnFinSlices * kRnFinSlices >= kRnMaxPartials, "a finish thread takes at most kRnFinSlices partials");

struct RnArgs {
    const void *x, *res, *dy, *dh_in, *w, *hin;
    void *h, *y, *dh, *dw;
    float* rstd;
    float* ws;
    int64_t ld_x, ld_res, ld_h, ld_y, ld_dy, ld_dh_in, ld_dh;
    int64_t N, nblk;
    int D;
    float eps;
};

template <class DT> __device__ __forceinline__ float rn_round(float v);
template <> __device__ __forceinline__ float rn_round<F32T>(float v) { return v; }
template <> __device__ __forceinline__ float rn_round<BF16T>(float v) { return bf2f(f2bf(v)); }

// A thread's share of one row: E elements as E / W units.
template <class DT, bool VEC, int TEAM, int E>
struct RnTile {
    static constexpr int W = DT::kEPV;
    static constexpr int NV = E / W;
    static constexpr int RPB = kRnThreads / TEAM;             // rows per workgroup pass
    static_assert(E % W == 0 && (TEAM == kWave || TEAM == kRnThreads), "tile shape");
    typedef typename DT::elem_t El;
    int tl, rib, D;
    __device__ __forceinline__ RnTile(int d) : tl(int(threadIdx.x) % TEAM), rib(int(threadIdx.x) / TEAM), D(d) {}
    __device__ __forceinline__ int col(int k) const { return (k * TEAM + tl) * W; }
    // elements past D read as 0
    __device__ __forceinline__ void load(const void* p, int64_t row_off, float (&f)[E]) const {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = col(k);
            float u[W];
            if constexpr (VEC) {
                if (c < D) {                                   // D is a multiple of W
                    DT::unpack(ld_stream(reinterpret_cast<const vec4u*>(static_cast<const El*>(p) + row_off + c)), u);
                } else {
#pragma unroll
                    for (int e = 0; e < W; ++e) u[e] = 0.f;
                }
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) u[e] = c + e < D ? DT::load1(p, row_off + c + e) : 0.f;
            }
#pragma unroll
            for (int e = 0; e < W; ++e) f[k * W + e] = u[e];
        }
    }
    __device__ __forceinline__ void store(void* p, int64_t row_off, const float (&f)[E]) const {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = col(k);
            if constexpr (VEC) {
                if (c < D) {
                    float u[W];
#pragma unroll
                    for (int e = 0; e < W; ++e) u[e] = f[k * W + e];
                    __builtin_nontemporal_store(DT::pack(u), reinterpret_cast<vec4u*>(static_cast<El*>(p) + row_off + c));
                }
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e)
                    if (c + e < D) DT::store1(p, row_off + c + e, f[k * W + e]);
            }
        }
    }
    // a team-wide sum, the same value in every thread of the team.  TEAM = 256: `sh` is 2 x 4 slots
    // used in turn, so that one barrier per sum is enough (a wave can be one sum ahead of another,
    // never two).
    __device__ __forceinline__ float sum(float v, float* sh, int& turn) const {
        v = wave_sum(v);
        if constexpr (TEAM == kWave) return v;
        float* s = sh + turn * (kRnThreads / kWave);
        turn ^= 1;
        if ((threadIdx.x & (kWave - 1)) == 0) s[threadIdx.x / kWave] = v;
        __syncthreads();
        return ((s[0] + s[1]) + s[2]) + s[3];
    }
};

template <class DT, bool VEC, int TEAM, int E>
__global__ __launch_bounds__(kRnThreads) void k_t5_rmsnorm_fwd(RnArgs k) {
    typedef RnTile<DT, VEC, TEAM, E> T;
    __shared__ float sh[2 * (kRnThreads / kWave)];
    const T t(k.D);
    int turn = 0;
    float w[E];
    t.load(k.w, 0, w);
#pragma unroll 1
    for (int64_t b = blockIdx.x; b < k.nblk; b += gridDim.x) {
        const int64_t row = b * T::RPB + t.rib;
        if (T::RPB > 1 && row >= k.N) continue;                // a whole wave: no barrier in this form
        float f[E];
        t.load(k.x, row * k.ld_x, f);
        if (k.res) {
            float r[E];
            t.load(k.res, row * k.ld_res, r);
#pragma unroll
            for (int i = 0; i < E; ++i) f[i] = rn_round<DT>(r[i] + f[i]);
            t.store(k.h, row * k.ld_h, f);
        }
        const float rstd = rn_rstd(t.sum(rn_sumsq(f), sh, turn), k.D, k.eps);
        if (k.rstd && t.tl == 0) k.rstd[row] = rstd;
#pragma unroll
        for (int i = 0; i < E; ++i) f[i] = w[i] * (f[i] * rstd);
        t.store(k.y, row * k.ld_y, f);
    }
}

template <class DT, bool VEC, int TEAM, int E, bool DH, bool DW>
__global__ __launch_bounds__(kRnThreads) void k_t5_rmsnorm_bwd(RnArgs k) {
    typedef RnTile<DT, VEC, TEAM, E> T;
    __shared__ float sh[2 * (kRnThreads / kWave)];
    __shared__ float shw[DW && T::RPB > 1 ? (T::RPB - 1) * E * TEAM : 1];
    const T t(k.D);
    int turn = 0;
    float w[DH ? E : 1], acc[DW ? E : 1];
    if constexpr (DH) t.load(k.w, 0, w);
    if constexpr (DW) {
#pragma unroll
        for (int i = 0; i < E; ++i) acc[i] = 0.f;
    }
#pragma unroll 1
    for (int64_t b = blockIdx.x; b < k.nblk; b += gridDim.x) {
        const int64_t row = b * T::RPB + t.rib;
        if (T::RPB > 1 && row >= k.N) continue;
        float fh[E], fg[E];
        t.load(k.hin, row * k.ld_h, fh);
        t.load(k.dy, row * k.ld_dy, fg);
        const float rstd = k.rstd ? k.rstd[row] : rn_rstd(t.sum(rn_sumsq(fh), sh, turn), k.D, k.eps);
#pragma unroll
        for (int i = 0; i < E; ++i) fh[i] *= rstd;             // hh
        if constexpr (DW) {
#pragma unroll
            for (int i = 0; i < E; ++i) acc[i] += fg[i] * fh[i];
        }
        if constexpr (DH) {
            float p = 0.f;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                fg[i] *= w[i];                                 // g
                p += fg[i] * fh[i];
            }
            const float c = t.sum(p, sh, turn) / float(k.D);
#pragma unroll
            for (int i = 0; i < E; ++i) fg[i] = rstd * (fg[i] - fh[i] * c);
            if (k.dh_in) {
                t.load(k.dh_in, row * k.ld_dh_in, fh);
#pragma unroll
                for (int i = 0; i < E; ++i) fg[i] += fh[i];
            }
            t.store(k.dh, row * k.ld_dh, fg);
        }
    }
    if constexpr (DW) {
        if constexpr (T::RPB > 1) {                            // waves 1.. park their sums, wave 0 adds them in order
            if (t.rib > 0) {
#pragma unroll
                for (int i = 0; i < E; ++i) shw[((t.rib - 1) * E + i) * TEAM + t.tl] = acc[i];
            }
            __syncthreads();
            if (t.rib > 0) return;
#pragma unroll
            for (int r = 0; r < T::RPB - 1; ++r)
#pragma unroll
                for (int i = 0; i < E; ++i) acc[i] += shw[(r * E + i) * TEAM + t.tl];
        }
        float* out = k.ws + int64_t(blockIdx.x) * k.D;
#pragma unroll
        for (int kk = 0; kk < T::NV; ++kk) {
            const int c = t.col(kk);
#pragma unroll
            for (int e = 0; e < T::W; ++e)
                if (c + e < k.D) out[c + e] = acc[kk * T::W + e];
        }
    }
}

// dw[j] = sum over the G partial rows, rounded once.  Thread (s, c) of a workgroup adds rows s, s + 32, ...
// of column c in row order (at most 32 loads, all in flight at once), then the 32 slice sums of a
// column are added in slice order.  Fixed order: bit-reproducible.
template <class DT>
__global__ __launch_bounds__(kRnFinCols * kRnFinSlices) void k_t5_rmsnorm_dw(const float* ws, void* dw, int D, int G) {
    __shared__ float sh[kRnFinSlices][kRnFinCols];
    const int c = int(threadIdx.x) % kRnFinCols, s = int(threadIdx.x) / kRnFinCols;
    const int col = int(blockIdx.x) * kRnFinCols + c;
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < kRnFinSlices; ++i) {
        const int g = s + i * kRnFinSlices;
        const bool in = g < G && col < D;                      // the address is clamped so that every load can be issued
        const float v = ws[int64_t(in ? g : 0) * D + (col < D ? col : 0)];
        a += in ? v : 0.f;
    }
    sh[s][c] = a;
    __syncthreads();
    if (s == 0 && col < D) {
        float r = sh[0][c];
#pragma unroll
        for (int j = 1; j < kRnFinSlices; ++j) r += sh[j][c];
        DT::store1(dw, col, r);
    }
}

typedef void (*rn_kernel_t)(RnArgs);

// form: index into kRnBreaks
template <class DT, bool VEC>
static rn_kernel_t rn_pick_fwd(int form) {
    switch (form) {
        case 0: return k_t5_rmsnorm_fwd<DT, VEC, kWave, 8>;
        case 1: return k_t5_rmsnorm_fwd<DT, VEC, kWave, 16>;
        case 2: return k_t5_rmsnorm_fwd<DT, VEC, kRnThreads, 8>;
        case 3: return k_t5_rmsnorm_fwd<DT, VEC, kRnThreads, 16>;
        default: return k_t5_rmsnorm_fwd<DT, VEC, kRnThreads, 32>;
    }
}

template <class DT, bool VEC, bool DH, bool DW>
static rn_kernel_t rn_pick_bwd_form(int form) {
    switch (form) {
        case 0: return k_t5_rmsnorm_bwd<DT, VEC, kWave, 8, DH, DW>;
        case 1: return k_t5_rmsnorm_bwd<DT, VEC, kWave, 16, DH, DW>;
        case 2: return k_t5_rmsnorm_bwd<DT, VEC, kRnThreads, 8, DH, DW>;
        case 3: return k_t5_rmsnorm_bwd<DT, VEC, kRnThreads, 16, DH, DW>;
        default: return k_t5_rmsnorm_bwd<DT, VEC, kRnThreads, 32, DH, DW>;
    }
}

template <class DT, bool VEC>
static rn_kernel_t rn_pick_bwd(int form, bool dh, bool dw) {
    if (dh && dw) return rn_pick_bwd_form<DT, VEC, true, true>(form);
    return dh ? rn_pick_bwd_form<DT, VEC, true, false>(form) : rn_pick_bwd_form<DT, VEC, false, true>(form);
}

static int rn_form(int64_t D) {
    int f = 0;
    while (f < 4 && D > kRnBreaks[f]) ++f;
    return f;
}
static int rn_rows_per_block(int64_t D) { return D <= kRnWaveMaxD ? kRnThreads / kWave : 1; }
static int64_t rn_row_blocks(int64_t N, int64_t D) { return (N + rn_rows_per_block(D) - 1) / rn_rows_per_block(D); }
static int64_t rn_partials(int64_t N, int64_t D) {
    const int64_t nb = rn_row_blocks(N, D);
    return nb < kRnMaxPartials ? nb : kRnMaxPartials;
}

// One operand of a call: N rows of D elements `ld` apart (ld 0: one vector of D elements, w / dw).
struct RnOp {
    const char* name;
    const void* base;
    int64_t ld;
    bool written;
    uintptr_t lo, hi;   // byte range, filled by rn_check
};

// The checks both entries share; *vec: every operand is on the 16-byte grid.
static int rn_check(const char* who, const TrlxT5RmsNormArgs* a, RnOp* ops, int nops, bool* vec) {
    TRLX_REQUIRE(a->dtype == TRLX_F32 || a->dtype == TRLX_BF16, TRLX_ERR_DTYPE, "%s: dtype %d (float32 and bfloat16 only)",
                 who, a->dtype);
    TRLX_REQUIRE(a->D >= 1 && a->D <= kRnMaxD, TRLX_ERR_SHAPE, "%s: D %lld (1 to %d: a row stays in registers)", who,
                 (long long)a->D, kRnMaxD);
    TRLX_REQUIRE(a->N >= 0 && a->N <= (int64_t(1) << 40), TRLX_ERR_SHAPE, "%s: N %lld (0 to 2^40)", who, (long long)a->N);
    TRLX_REQUIRE(a->eps == a->eps, TRLX_ERR_ARG, "%s: eps is NaN", who);
    const int64_t esz = a->dtype == TRLX_BF16 ? 2 : 4, w = 16 / esz;
    bool v16 = a->D % w == 0;
    for (int i = 0; i < nops; ++i) {
        RnOp& op = ops[i];
        const uintptr_t p = reinterpret_cast<uintptr_t>(op.base);
        TRLX_REQUIRE(p % uintptr_t(esz) == 0, TRLX_ERR_ARG, "%s: %s not aligned to its element", who, op.name);
        int64_t span = 0;
        if (op.ld != 0) {
            TRLX_REQUIRE(op.ld >= a->D, TRLX_ERR_STRIDE, "%s: %s row stride %lld below D = %lld", who, op.name,
                         (long long)op.ld, (long long)a->D);
            TRLX_REQUIRE(!__builtin_mul_overflow(a->N > 0 ? a->N - 1 : 0, op.ld, &span) && span <= (int64_t(1) << 59),
                         TRLX_ERR_STRIDE, "%s: %s rows %lld apart do not fit the address space", who, op.name, (long long)op.ld);
        }
        op.lo = p, op.hi = p + uintptr_t((span + a->D) * esz);
        v16 = v16 && p % 16 == 0 && op.ld % w == 0;
    }
    *vec = v16;
    return TRLX_OK;
}

// A written operand shares no byte range with another operand, except that it may be the very rows
// (same base, same stride) of one of `same`: every thread reads its elements of a row before it
// writes them.
static int rn_no_overlap(const char* who, const RnOp* ops, int nops, const char* written, const char* const* same, int nsame) {
    const RnOp* x = nullptr;
    for (int i = 0; i < nops; ++i)
        if (!strcmp(ops[i].name, written)) x = &ops[i];
    if (!x) return TRLX_OK;
    for (int i = 0; i < nops; ++i) {
        const RnOp& y = ops[i];
        if (&y == x || x->hi <= y.lo || y.hi <= x->lo) continue;
        bool ok = false;
        for (int s = 0; s < nsame; ++s) ok = ok || (!strcmp(y.name, same[s]) && y.base == x->base && y.ld == x->ld);
        TRLX_REQUIRE(ok, TRLX_ERR_ARG, "%s: %s overlaps %s", who, x->name, y.name);
    }
    return TRLX_OK;
}

// ------------------------------------------------------------------ the decoder's input row of a decode step
// trlx_t5_decode_embed: h[b, :] = weight[tok_b, :] with tok_b the token drawn at step t - 1 (the
// start token at t = 0), and, with a norm weight, y[b, :] = the forward above on that row -- the
// same RnTile, the same sum, rn_rstd and the same product, so y has the bits of k_t5_rmsnorm_fwd on
// h.  The row stays in registers between the gather and the two stores.
struct EmbArgs {
    const void* weight;
    const int64_t* tokens;
    const void* w;          // the norm weight or NULL
    void *h, *y;
    int64_t ld_w, ld_tokens, ld_h, ld_y;
    int64_t B, nblk, V, T, t, start;
    int D;
    float eps;
};
// The device-clock step: t comes from the decode clock, a.t is not read.
struct EmbDevArgs {
    EmbArgs a;
    const int64_t* clock;
};
__device__ __forceinline__ const EmbArgs& emb_args(const EmbArgs& a) { return a; }
__device__ __forceinline__ const EmbArgs& emb_args(const EmbDevArgs& a) { return a.a; }

// DEVT: t and the capacity are loaded from the clock once, at the top of the workgroup.  The step is
// live iff 0 <= t < capacity and t - 1 < T (the columns of `tokens`); a dead step stores zeros to h
// and y and leaves, before any address is formed from t and before any barrier (the exit is
// uniform).  A token outside [0, V) is tested before any address is formed from it: a zero row.
template <class DT, bool VEC, int TEAM, int E, bool NORM, bool DEVT>
__global__ __launch_bounds__(kRnThreads) void k_t5_decode_embed(const std::conditional_t<DEVT, EmbDevArgs, EmbArgs> args) {
    typedef RnTile<DT, VEC, TEAM, E> T;
    __shared__ float sh[2 * (kRnThreads / kWave)];
    const EmbArgs& k = emb_args(args);
    const T t(k.D);
    int64_t step = k.t;
    if constexpr (DEVT) {
        const int64_t tc = args.clock[TRLX_CLOCK_T], cap = args.clock[TRLX_CLOCK_CAP];
        if (tc < 0 || tc >= cap || tc - 1 >= k.T) {   // block-uniform
            float z[E];
#pragma unroll
            for (int i = 0; i < E; ++i) z[i] = 0.f;
#pragma unroll 1
            for (int64_t b = blockIdx.x; b < k.nblk; b += gridDim.x) {
                const int64_t row = b * T::RPB + t.rib;
                if (T::RPB > 1 && row >= k.B) continue;
                t.store(k.h, row * k.ld_h, z);
                if constexpr (NORM) t.store(k.y, row * k.ld_y, z);
            }
            return;
        }
        step = tc;
    }
    int turn = 0;
    float w[NORM ? E : 1];
    if constexpr (NORM) t.load(k.w, 0, w);
#pragma unroll 1
    for (int64_t b = blockIdx.x; b < k.nblk; b += gridDim.x) {
        const int64_t row = b * T::RPB + t.rib;
        if (T::RPB > 1 && row >= k.B) continue;                // a whole wave: no barrier in this form
        const int64_t tok = step == 0 ? k.start : k.tokens[row * k.ld_tokens + step - 1];
        float f[E];
        if (tok >= 0 && tok < k.V) {                           // uniform over the row's team
            t.load(k.weight, tok * k.ld_w, f);
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) f[i] = 0.f;
        }
        t.store(k.h, row * k.ld_h, f);
        if constexpr (NORM) {
            const float rstd = rn_rstd(t.sum(rn_sumsq(f), sh, turn), k.D, k.eps);
#pragma unroll
            for (int i = 0; i < E; ++i) f[i] = w[i] * (f[i] * rstd);
            t.store(k.y, row * k.ld_y, f);
        }
    }
}

template <bool DEVT>
using emb_kernel_t = void (*)(const std::conditional_t<DEVT, EmbDevArgs, EmbArgs>);

template <class DT, bool VEC, bool NORM, bool DEVT>
static emb_kernel_t<DEVT> emb_pick_form(int form) {
    switch (form) {
        case 0: return k_t5_decode_embed<DT, VEC, kWave, 8, NORM, DEVT>;
        case 1: return k_t5_decode_embed<DT, VEC, kWave, 16, NORM, DEVT>;
        case 2: return k_t5_decode_embed<DT, VEC, kRnThreads, 8, NORM, DEVT>;
        case 3: return k_t5_decode_embed<DT, VEC, kRnThreads, 16, NORM, DEVT>;
        default: return k_t5_decode_embed<DT, VEC, kRnThreads, 32, NORM, DEVT>;
    }
}
template <bool DEVT>
static emb_kernel_t<DEVT> emb_pick(bool bf, int form, bool vec, bool norm) {
    if (bf) {
        if (vec) return norm ? emb_pick_form<BF16T, true, true, DEVT>(form) : emb_pick_form<BF16T, true, false, DEVT>(form);
        return norm ? emb_pick_form<BF16T, false, true, DEVT>(form) : emb_pick_form<BF16T, false, false, DEVT>(form);
    }
    if (vec) return norm ? emb_pick_form<F32T, true, true, DEVT>(form) : emb_pick_form<F32T, true, false, DEVT>(form);
    return norm ? emb_pick_form<F32T, false, true, DEVT>(form) : emb_pick_form<F32T, false, false, DEVT>(form);
}

// One operand of trlx_t5_decode_embed as a byte range.
struct EmbOp {
    const char* name;
    uintptr_t lo, hi;
    bool written;
};

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_decode_embed(const TrlxT5DecodeEmbedArgs* a, const int64_t* clock, void* stream) {
    const char* who = "t5 decode embed";
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->dtype == TRLX_F32 || a->dtype == TRLX_BF16, TRLX_ERR_DTYPE, "%s: dtype %d (float32 and bfloat16 only)",
                 who, a->dtype);
    TRLX_REQUIRE(a->D >= 1 && a->D <= kRnMaxD, TRLX_ERR_SHAPE, "%s: D %lld (1 to %d: a row stays in registers)", who,
                 (long long)a->D, kRnMaxD);
    TRLX_REQUIRE(a->B >= 1 && a->B <= 0x7fffffffLL && a->V >= 1 && a->V <= 0x7fffffffLL && a->T >= 1 &&
                     a->T <= 0x7fffffffLL,
                 TRLX_ERR_SHAPE, "%s: B %lld, V %lld, T %lld (1 to 2^31 - 1 each)", who, (long long)a->B, (long long)a->V,
                 (long long)a->T);
    TRLX_REQUIRE(a->weight && a->tokens && a->h, TRLX_ERR_ARG, "%s: NULL weight / tokens / h", who);
    TRLX_REQUIRE((a->y != nullptr) == (a->norm_w != nullptr), TRLX_ERR_ARG,
                 "%s: y and norm_w go together (without a norm weight only h is written)", who);
    TRLX_REQUIRE(a->eps == a->eps, TRLX_ERR_ARG, "%s: eps is NaN", who);
    TRLX_REQUIRE(clock || (a->t >= 0 && a->t <= a->T), TRLX_ERR_ARG, "%s: t %lld outside [0, T = %lld]", who,
                 (long long)a->t, (long long)a->T);
    const int64_t esz = a->dtype == TRLX_BF16 ? 2 : 4, vw = 16 / esz;
    const bool norm = a->norm_w != nullptr;
    const int64_t ld_y = norm ? a->ld_y : a->D;
    TRLX_REQUIRE(a->ld_w >= a->D && a->ld_h >= a->D && ld_y >= a->D, TRLX_ERR_STRIDE,
                 "%s: row strides %lld (weight), %lld (h), %lld (y) below D = %lld", who, (long long)a->ld_w,
                 (long long)a->ld_h, (long long)ld_y, (long long)a->D);
    TRLX_REQUIRE(a->ld_tokens >= a->T, TRLX_ERR_STRIDE, "%s: tokens row stride %lld below T = %lld", who,
                 (long long)a->ld_tokens, (long long)a->T);
    TRLX_REQUIRE(a->ld_w <= (int64_t(1) << 28) && a->ld_h <= (int64_t(1) << 28) && ld_y <= (int64_t(1) << 28) &&
                     a->ld_tokens <= (int64_t(1) << 28),
                 TRLX_ERR_STRIDE, "%s: rows that far apart do not fit the address space", who);
    const uintptr_t pw = reinterpret_cast<uintptr_t>(a->weight), ph = reinterpret_cast<uintptr_t>(a->h),
                    py = reinterpret_cast<uintptr_t>(a->y), pn = reinterpret_cast<uintptr_t>(a->norm_w),
                    pt = reinterpret_cast<uintptr_t>(a->tokens), pc = reinterpret_cast<uintptr_t>(clock);
    TRLX_REQUIRE(pw % uintptr_t(esz) == 0 && ph % uintptr_t(esz) == 0 && py % uintptr_t(esz) == 0 &&
                     pn % uintptr_t(esz) == 0,
                 TRLX_ERR_ARG, "%s: weight / h / y / norm_w not aligned to the element", who);
    TRLX_REQUIRE(pt % 8 == 0 && pc % 8 == 0, TRLX_ERR_ARG, "%s: tokens / clock not aligned to 8 bytes", who);
    EmbOp ops[6];
    int n = 0;
    ops[n++] = {"weight", pw, pw + uintptr_t(((a->V - 1) * a->ld_w + a->D) * esz), false};
    ops[n++] = {"tokens", pt, pt + uintptr_t(((a->B - 1) * a->ld_tokens + a->T) * 8), false};
    ops[n++] = {"h", ph, ph + uintptr_t(((a->B - 1) * a->ld_h + a->D) * esz), true};
    if (norm) {
        ops[n++] = {"y", py, py + uintptr_t(((a->B - 1) * ld_y + a->D) * esz), true};
        ops[n++] = {"norm_w", pn, pn + uintptr_t(a->D * esz), false};
    }
    if (clock) ops[n++] = {"clock", pc, pc + uintptr_t(TRLX_CLOCK_WORDS * 8), false};
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            TRLX_REQUIRE(i == j || !ops[i].written || ops[i].hi <= ops[j].lo || ops[j].hi <= ops[i].lo, TRLX_ERR_ARG,
                         "%s: %s overlaps %s", who, ops[i].name, ops[j].name);
    const bool vec = a->D % vw == 0 && pw % 16 == 0 && ph % 16 == 0 && py % 16 == 0 && pn % 16 == 0 &&
                     a->ld_w % vw == 0 && a->ld_h % vw == 0 && ld_y % vw == 0;
    EmbDevArgs k = {};
    k.a.weight = a->weight, k.a.tokens = a->tokens, k.a.w = a->norm_w, k.a.h = a->h, k.a.y = a->y;
    k.a.ld_w = a->ld_w, k.a.ld_tokens = a->ld_tokens, k.a.ld_h = a->ld_h, k.a.ld_y = ld_y;
    k.a.B = a->B, k.a.nblk = rn_row_blocks(a->B, a->D), k.a.V = a->V, k.a.T = a->T, k.a.t = clock ? 0 : a->t;
    k.a.start = a->start_token_id, k.a.D = int(a->D), k.a.eps = a->eps;
    k.clock = clock;
    const int form = rn_form(a->D);
    const dim3 grid(unsigned(rn_partials(a->B, a->D))), block(kRnThreads);
    const bool bf = a->dtype == TRLX_BF16;
    if (clock)
        hipLaunchKernelGGL(emb_pick<true>(bf, form, vec, norm), grid, block, 0, (hipStream_t)stream, k);
    else
        hipLaunchKernelGGL(emb_pick<false>(bf, form, vec, norm), grid, block, 0, (hipStream_t)stream, k.a);
    return check_launch("k_t5_decode_embed");
}

extern "C" int trlx_t5_rmsnorm_geometry(int64_t N, int64_t D, TrlxT5RmsNormGeometry* g) {
    TRLX_REQUIRE(g, TRLX_ERR_ARG, "t5 rmsnorm geometry: NULL result");
    TRLX_REQUIRE(N >= 0 && D >= 0, TRLX_ERR_SHAPE, "t5 rmsnorm geometry: N %lld, D %lld", (long long)N, (long long)D);
    *g = TrlxT5RmsNormGeometry{};
    g->vec_bf16 = BF16T::kEPV, g->vec_f32 = F32T::kEPV;
    g->threads = kRnThreads;
    g->max_partials = kRnMaxPartials;
    g->max_d = g->reg_max_d = kRnMaxD;
    g->wave_row_max_d = kRnWaveMaxD;
    g->n_breaks = 5;
    for (int i = 0; i < 5; ++i) g->d_breaks[i] = kRnBreaks[i];
    if (D >= 1 && D <= kRnMaxD) {
        g->rows_per_block = rn_rows_per_block(D);
        g->row_blocks = rn_row_blocks(N, D);
        g->partials = rn_partials(N, D);
        g->ws_bytes = g->partials * D * 4;
    }
    return TRLX_OK;
}

extern "C" int trlx_t5_rmsnorm_fwd(const TrlxT5RmsNormArgs* a, void* stream) {
    const char* who = "t5 rmsnorm fwd";
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->x && a->y && a->w, TRLX_ERR_ARG, "%s: NULL x / y / w", who);
    TRLX_REQUIRE((a->residual != nullptr) == (a->h != nullptr), TRLX_ERR_ARG,
                 "%s: residual and h go together (the add form writes h; without residual, x is h)", who);
    TRLX_REQUIRE(!a->rstd || reinterpret_cast<uintptr_t>(a->rstd) % 4 == 0, TRLX_ERR_ARG, "%s: rstd not aligned to 4 bytes", who);
    RnOp ops[5];
    int n = 0;
    ops[n++] = {"x", a->x, a->ld_x, false, 0, 0};
    if (a->residual) ops[n++] = {"residual", a->residual, a->ld_residual, false, 0, 0};
    if (a->h) ops[n++] = {"h", a->h, a->ld_h, true, 0, 0};
    ops[n++] = {"y", a->y, a->ld_y, true, 0, 0};
    ops[n++] = {"w", a->w, 0, false, 0, 0};
    bool vec;
    int rc = rn_check(who, a, ops, n, &vec);
    if (rc != TRLX_OK || a->N == 0) return rc;
    const char* h_same[] = {"x", "residual"};
    if ((rc = rn_no_overlap(who, ops, n, "h", h_same, 2)) != TRLX_OK) return rc;
    const char* y_same[] = {"x"};
    if ((rc = rn_no_overlap(who, ops, n, "y", y_same, a->residual ? 0 : 1)) != TRLX_OK) return rc;
    RnArgs k = {};
    k.x = a->x, k.res = a->residual, k.w = a->w, k.h = a->h, k.y = a->y, k.rstd = static_cast<float*>(a->rstd);
    k.ld_x = a->ld_x, k.ld_res = a->ld_residual, k.ld_h = a->ld_h, k.ld_y = a->ld_y;
    k.N = a->N, k.D = int(a->D), k.eps = a->eps, k.nblk = rn_row_blocks(a->N, a->D);
    const int form = rn_form(a->D);
    const rn_kernel_t fn = a->dtype == TRLX_BF16 ? (vec ? rn_pick_fwd<BF16T, true>(form) : rn_pick_fwd<BF16T, false>(form))
                                                 : (vec ? rn_pick_fwd<F32T, true>(form) : rn_pick_fwd<F32T, false>(form));
    hipLaunchKernelGGL(fn, dim3(unsigned(rn_partials(a->N, a->D))), dim3(kRnThreads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_rmsnorm_fwd");
}

extern "C" int trlx_t5_rmsnorm_bwd(const TrlxT5RmsNormArgs* a, void* stream) {
    const char* who = "t5 rmsnorm bwd";
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->h && a->dy, TRLX_ERR_ARG, "%s: NULL h / dy", who);
    TRLX_REQUIRE(a->dh || a->dw, TRLX_ERR_ARG, "%s: neither dh nor dw asked for", who);
    TRLX_REQUIRE(!a->dh || a->w, TRLX_ERR_ARG, "%s: dh needs w", who);
    TRLX_REQUIRE(!a->dh_in || a->dh, TRLX_ERR_ARG, "%s: dh_in with no dh", who);
    TRLX_REQUIRE(!a->rstd || reinterpret_cast<uintptr_t>(a->rstd) % 4 == 0, TRLX_ERR_ARG, "%s: rstd not aligned to 4 bytes", who);
    RnOp ops[6];
    int n = 0;
    ops[n++] = {"h", a->h, a->ld_h, false, 0, 0};
    ops[n++] = {"dy", a->dy, a->ld_dy, false, 0, 0};
    if (a->dh_in) ops[n++] = {"dh_in", a->dh_in, a->ld_dh_in, false, 0, 0};
    if (a->dh) ops[n++] = {"dh", a->dh, a->ld_dh, true, 0, 0};
    if (a->dh) ops[n++] = {"w", a->w, 0, false, 0, 0};
    if (a->dw) ops[n++] = {"dw", a->dw, 0, true, 0, 0};
    bool vec;
    int rc = rn_check(who, a, ops, n, &vec);
    if (rc != TRLX_OK) return rc;
    const int64_t G = rn_partials(a->N, a->D), need = G * a->D * 4;
    if (a->dw && a->N > 0)
        TRLX_REQUIRE(a->ws && reinterpret_cast<uintptr_t>(a->ws) % 4 == 0 && a->ws_bytes >= need, TRLX_ERR_ARG,
                     "%s: workspace of %lld bytes, %lld needed (4-byte aligned)", who, (long long)a->ws_bytes, (long long)need);
    const char* dh_same[] = {"dh_in", "dy"};
    if ((rc = rn_no_overlap(who, ops, n, "dh", dh_same, 2)) != TRLX_OK) return rc;
    if ((rc = rn_no_overlap(who, ops, n, "dw", nullptr, 0)) != TRLX_OK) return rc;
    const bool bf = a->dtype == TRLX_BF16;
    if (a->N == 0) {                                           // an empty sum: dw = 0
        if (a->dw && hipMemsetAsync(a->dw, 0, size_t(a->D) * (bf ? 2 : 4), (hipStream_t)stream) != hipSuccess)
            return check_launch("t5 rmsnorm bwd: dw of no rows");
        return TRLX_OK;
    }
    RnArgs k = {};
    k.hin = a->h, k.dy = a->dy, k.dh_in = a->dh_in, k.w = a->w, k.dh = a->dh, k.dw = a->dw;
    k.rstd = static_cast<float*>(a->rstd), k.ws = static_cast<float*>(a->ws);
    k.ld_h = a->ld_h, k.ld_dy = a->ld_dy, k.ld_dh_in = a->ld_dh_in, k.ld_dh = a->ld_dh;
    k.N = a->N, k.D = int(a->D), k.eps = a->eps, k.nblk = rn_row_blocks(a->N, a->D);
    const int form = rn_form(a->D);
    const bool dh = a->dh != nullptr, dw = a->dw != nullptr;
    const rn_kernel_t fn = bf ? (vec ? rn_pick_bwd<BF16T, true>(form, dh, dw) : rn_pick_bwd<BF16T, false>(form, dh, dw))
                              : (vec ? rn_pick_bwd<F32T, true>(form, dh, dw) : rn_pick_bwd<F32T, false>(form, dh, dw));
    hipLaunchKernelGGL(fn, dim3(unsigned(G)), dim3(kRnThreads), 0, (hipStream_t)stream, k);
    rc = check_launch("k_t5_rmsnorm_bwd");
    if (rc != TRLX_OK || !dw) return rc;
    const unsigned fin = unsigned((a->D + kRnFinCols - 1) / kRnFinCols);
    if (bf)
        hipLaunchKernelGGL(k_t5_rmsnorm_dw<BF16T>, dim3(fin), dim3(kRnFinCols * kRnFinSlices), 0, (hipStream_t)stream, k.ws, a->dw, k.D, int(G));
    else
        hipLaunchKernelGGL(k_t5_rmsnorm_dw<F32T>, dim3(fin), dim3(kRnFinCols * kRnFinSlices), 0, (hipStream_t)stream, k.ws, a->dw, k.D, int(G));
    return check_launch("k_t5_rmsnorm_dw");
}
