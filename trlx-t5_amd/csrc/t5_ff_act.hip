// T5 feed-forward activation (HF T5DenseGatedActDense / T5DenseActDense between the projections):
//   forward   out = act(u) * v            (out = act(u) when not gated)
//   backward  du = dy * v * act'(u),  dv = dy * act(u)      one launch, act(u) recomputed
// HBM-bound row work: no reductions, no cross-lane traffic, no LDS.  One workgroup of 4 waves takes
// a block of kFaRows x kFaCols elements; a wave takes 4 rows of it, 1 KB (bf16) or 2 KB (fp32) of
// each operand per row in 16-byte lane accesses, four vectors of every operand in flight per lane
// before the first is used.  Operands that break the 16-byte rule take the same block shape with
// element accesses (VEC = false); both forms run the same fa_eval on the same fp32 values.
//
// gelu_new and silu are u * sigmoid(x) with x = u (silu) or x = 2 sqrt(2/pi) (u + 0.044715 u^3)
// (gelu_new: 0.5 (1 + tanh(z)) = sigmoid(2z)).  From e = exp(-|x|) in (0, 1] and r = 1 / (1 + e):
//   sigmoid(x) = r (x >= 0) or e r (x < 0),     sigmoid'(x) = e r^2
// so nothing is subtracted: 1 + tanh(z) would lose the negative tail, 1 - sigmoid the positive one.
// e is v_exp_f32 of -|x| log2(e) and r is v_rcp_f32 (1 ulp each); the rounding of the product
// |x| log2(e) moves e by a relative |x| 2^-24, and e |x| <= 1/e, so every result stays within a
// few fp32 ulps of its own size plus about 2^-25 of |u| (act) or of 1 (act') — two orders inside
// the 2^-16 floor the tests allow, at about a third of the VALU work of expf and an IEEE divide.
// Overflow: u^2 may be +inf (|u| > 1.8e19); then x = +-inf, e = 0, sigmoid' = 0 exactly, and the
// derivative's u x' sigmoid'(x) term (inf * 0) is replaced by the 0 it tends to.
#include "common.h"
#include "t5_row_math.h"

namespace trlx {

constexpr int kFaThreads = 256;
constexpr int kFaCols = 512;                                   // columns per workgroup
constexpr int kFaWaveRows = 4;                                 // rows per wave
constexpr int kFaRows = (kFaThreads / kWave) * kFaWaveRows;    // rows per workgroup

struct FaArgs {
    const void *u, *v, *dy;
    void *out, *du, *dv;
    int64_t ld_u, ld_v, ld_out, ld_dy, ld_du, ld_dv;
    int64_t N, F;
    unsigned nct;   // column blocks per row block
};

// One access: a 16-byte vector of the row (VEC) or one element.
template <class DT, bool VEC>
struct FaUnit {
    static constexpr int W = VEC ? DT::kEPV : 1;
    typedef typename DT::elem_t E;
    __device__ static __forceinline__ void load(const void* p, int64_t off, float (&f)[W]) {
        if constexpr (VEC)
            DT::unpack(ld_stream(reinterpret_cast<const vec4u*>(static_cast<const E*>(p) + off)), f);
        else
            f[0] = DT::load1(p, off);
    }
    __device__ static __forceinline__ void store(void* p, int64_t off, const float (&f)[W]) {
        if constexpr (VEC)
            __builtin_nontemporal_store(DT::pack(f), reinterpret_cast<vec4u*>(static_cast<E*>(p) + off));
        else
            DT::store1(p, off, f[0]);
    }
};

// The block's accesses: item `it` of a wave is access it % UPR of its row it / UPR.
template <class DT, bool VEC>
struct FaTile {
    typedef FaUnit<DT, VEC> U;
    static constexpr int W = U::W;
    static constexpr int UPR = kFaCols / (kWave * W);          // accesses per lane and row
    static constexpr int ITEMS = kFaWaveRows * UPR;
    static constexpr int B = VEC ? 4 : 8;                      // accesses in flight per operand
    static_assert(kFaCols % (kWave * W) == 0 && ITEMS % B == 0, "block shape");
    int64_t row0, col0;
    int lane;
    __device__ __forceinline__ FaTile(unsigned nct) {
        const unsigned rt = blockIdx.x / nct;
        col0 = int64_t(blockIdx.x - rt * nct) * kFaCols;
        row0 = int64_t(rt) * kFaRows + int(threadIdx.x / kWave) * kFaWaveRows;
        lane = int(threadIdx.x & (kWave - 1));
    }
    __device__ __forceinline__ int64_t row(int it) const { return row0 + it / UPR; }
    __device__ __forceinline__ int64_t col(int it) const { return col0 + int64_t((it % UPR) * kWave + lane) * W; }
};

template <class DT, int ACT, bool GATED, bool VEC>
__global__ __launch_bounds__(kFaThreads) void k_t5_ff_act_fwd(FaArgs k) {
    typedef FaTile<DT, VEC> T;
    typedef typename T::U U;
    constexpr int W = T::W, B = T::B;
    const T t(k.nct);
#pragma unroll 1
    for (int it0 = 0; it0 < T::ITEMS; it0 += B) {
        float fu[B][W], fv[B][W];
        int64_t r[B], c[B];
        bool ok[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            r[b] = t.row(it0 + b), c[b] = t.col(it0 + b);
            ok[b] = r[b] < k.N && c[b] < k.F;                   // VEC: F is a multiple of W
            if (ok[b]) {
                U::load(k.u, r[b] * k.ld_u + c[b], fu[b]);
                if (GATED) U::load(k.v, r[b] * k.ld_v + c[b], fv[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (!ok[b]) continue;
            float y[W];
#pragma unroll
            for (int e = 0; e < W; ++e) {
                float a, d;
                fa_eval<ACT, false>(fu[b][e], a, d);
                y[e] = GATED ? a * fv[b][e] : a;
            }
            U::store(k.out, r[b] * k.ld_out + c[b], y);
        }
    }
}

// MODE: which gradients the launch writes
enum { kFaDu = 0, kFaDuDv = 1, kFaGatedDu = 2, kFaDv = 3 };   // kFaDu: not gated

template <class DT, int ACT, int MODE, bool VEC>
__global__ __launch_bounds__(kFaThreads) void k_t5_ff_act_bwd(FaArgs k) {
    typedef FaTile<DT, VEC> T;
    typedef typename T::U U;
    constexpr int W = T::W, B = T::B;
    constexpr bool DU = MODE != kFaDv, DV = MODE == kFaDuDv || MODE == kFaDv;
    constexpr bool READ_V = MODE == kFaDuDv || MODE == kFaGatedDu;
    const T t(k.nct);
#pragma unroll 1
    for (int it0 = 0; it0 < T::ITEMS; it0 += B) {
        float fg[B][W], fu[B][W], fv[B][W];
        int64_t r[B], c[B];
        bool ok[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            r[b] = t.row(it0 + b), c[b] = t.col(it0 + b);
            ok[b] = r[b] < k.N && c[b] < k.F;
            if (ok[b]) {
                U::load(k.dy, r[b] * k.ld_dy + c[b], fg[b]);
                U::load(k.u, r[b] * k.ld_u + c[b], fu[b]);
                if (READ_V) U::load(k.v, r[b] * k.ld_v + c[b], fv[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (!ok[b]) continue;
            float gu[W], gv[W];
#pragma unroll
            for (int e = 0; e < W; ++e) {
                float a, d;
                fa_eval<ACT, DU>(fu[b][e], a, d);
                if (DU) gu[e] = READ_V ? (fg[b][e] * fv[b][e]) * d : fg[b][e] * d;
                if (DV) gv[e] = fg[b][e] * a;
            }
            if (DU) U::store(k.du, r[b] * k.ld_du + c[b], gu);
            if (DV) U::store(k.dv, r[b] * k.ld_dv + c[b], gv);
        }
    }
}

typedef void (*fa_kernel_t)(FaArgs);

template <class DT, bool VEC>
static fa_kernel_t fa_pick_fwd(int act, bool gated) {
    switch (act) {
        case TRLX_T5_ACT_RELU:
            return gated ? k_t5_ff_act_fwd<DT, TRLX_T5_ACT_RELU, true, VEC> : k_t5_ff_act_fwd<DT, TRLX_T5_ACT_RELU, false, VEC>;
        case TRLX_T5_ACT_GELU_NEW:
            return gated ? k_t5_ff_act_fwd<DT, TRLX_T5_ACT_GELU_NEW, true, VEC>
                         : k_t5_ff_act_fwd<DT, TRLX_T5_ACT_GELU_NEW, false, VEC>;
        default:
            return gated ? k_t5_ff_act_fwd<DT, TRLX_T5_ACT_SILU, true, VEC> : k_t5_ff_act_fwd<DT, TRLX_T5_ACT_SILU, false, VEC>;
    }
}

template <class DT, int ACT, bool VEC>
static fa_kernel_t fa_pick_bwd_mode(int mode) {
    switch (mode) {
        case kFaDu: return k_t5_ff_act_bwd<DT, ACT, kFaDu, VEC>;
        case kFaDuDv: return k_t5_ff_act_bwd<DT, ACT, kFaDuDv, VEC>;
        case kFaGatedDu: return k_t5_ff_act_bwd<DT, ACT, kFaGatedDu, VEC>;
        default: return k_t5_ff_act_bwd<DT, ACT, kFaDv, VEC>;
    }
}

template <class DT, bool VEC>
static fa_kernel_t fa_pick_bwd(int act, int mode) {
    switch (act) {
        case TRLX_T5_ACT_RELU: return fa_pick_bwd_mode<DT, TRLX_T5_ACT_RELU, VEC>(mode);
        case TRLX_T5_ACT_GELU_NEW: return fa_pick_bwd_mode<DT, TRLX_T5_ACT_GELU_NEW, VEC>(mode);
        default: return fa_pick_bwd_mode<DT, TRLX_T5_ACT_SILU, VEC>(mode);
    }
}

// One operand of a call: rows of F elements, `ld` apart.
struct FaOp {
    const char* name;
    const void* base;
    int64_t ld;
    bool written;
    int64_t span;   // elements from the first to one past the last
};

// The checks both entries share; fills nct (0 with *launch = false for N == 0) and *vec.
static int fa_check(const char* who, const TrlxT5FfActArgs* a, FaOp* ops, int nops, unsigned* nct, bool* vec,
                    bool* launch) {
    TRLX_REQUIRE(a->dtype == TRLX_F32 || a->dtype == TRLX_BF16, TRLX_ERR_DTYPE, "%s: dtype %d (float32 and bfloat16 only)",
                 who, a->dtype);
    TRLX_REQUIRE(a->act == TRLX_T5_ACT_RELU || a->act == TRLX_T5_ACT_GELU_NEW || a->act == TRLX_T5_ACT_SILU, TRLX_ERR_ARG,
                 "%s: activation %d (relu 0, gelu_new 1, silu 2)", who, a->act);
    const int64_t lim = int64_t(1) << 40;
    TRLX_REQUIRE(a->F >= 1 && a->N >= 0 && a->F <= lim && a->N <= lim, TRLX_ERR_SHAPE, "%s: N %lld, F %lld (N in [0, 2^40], F in [1, 2^40])",
                 who, (long long)a->N, (long long)a->F);
    const int64_t esz = a->dtype == TRLX_BF16 ? 2 : 4, w = 16 / esz;
    bool v16 = a->F % w == 0;
    for (int i = 0; i < nops; ++i) {
        FaOp& op = ops[i];
        TRLX_REQUIRE(op.ld >= a->F, TRLX_ERR_STRIDE, "%s: %s row stride %lld below F = %lld", who, op.name, (long long)op.ld,
                     (long long)a->F);
        TRLX_REQUIRE(!__builtin_mul_overflow(a->N > 0 ? a->N - 1 : 0, op.ld, &op.span) && op.span <= (int64_t(1) << 59),
                     TRLX_ERR_STRIDE, "%s: %s rows %lld apart do not fit the address space", who, op.name, (long long)op.ld);
        op.span += a->F;
        const uintptr_t p = reinterpret_cast<uintptr_t>(op.base);
        TRLX_REQUIRE(p % uintptr_t(esz) == 0, TRLX_ERR_ARG, "%s: %s not aligned to its element", who, op.name);
        v16 = v16 && p % 16 == 0 && op.ld % w == 0;
    }
    const int64_t nrt = (a->N + kFaRows - 1) / kFaRows, nc = (a->F + kFaCols - 1) / kFaCols;
    TRLX_REQUIRE(nc <= 0x7fffffffLL && nrt <= 0x7fffffffLL && nrt * nc <= 0x7fffffffLL, TRLX_ERR_SHAPE, "%s: %lld x %lld blocks exceed the grid", who,
                 (long long)nrt, (long long)nc);
    *launch = a->N > 0;
    *nct = unsigned(nc);
    *vec = v16;
    if (a->N == 0) return TRLX_OK;
    // A written operand may not share an element with any other operand.  Address ranges apart: fine.
    // Ranges that interleave (the halves of one packed buffer) are taken only between operands of equal
    // row stride, where the rows can be told apart exactly: X's row i and Y's row j, `rem` elements
    // after X's base plus (j - i) ld, meet when that distance is inside (-F, F).
    for (int x = 0; x < nops; ++x) {
        if (!ops[x].written) continue;
        for (int y = 0; y < nops; ++y) {
            if (y == x || (ops[y].written && y < x)) continue;
            const FaOp &X = ops[x], &Y = ops[y];
            const uintptr_t x0 = reinterpret_cast<uintptr_t>(X.base), y0 = reinterpret_cast<uintptr_t>(Y.base);
            const uintptr_t xb = uintptr_t(X.span * esz), yb = uintptr_t(Y.span * esz);
            if (x0 + xb <= y0 || y0 + yb <= x0) continue;
            bool meet = true;
            if (a->N == 1 || X.ld == Y.ld) {
                const int64_t rem = (int64_t(y0) - int64_t(x0)) / esz;   // both aligned to esz: exact
                meet = false;
                if (a->N == 1) {
                    meet = rem > -a->F && rem < a->F;
                } else {
                    int64_t c0 = rem / X.ld;
                    if (rem % X.ld < 0) --c0;
                    for (int64_t c = c0; c <= c0 + 1; ++c) {
                        const int64_t d = rem - c * X.ld;
                        if (c > -a->N && c < a->N && d > -a->F && d < a->F) meet = true;
                    }
                }
            }
            TRLX_REQUIRE(!meet, TRLX_ERR_ARG,
                         "%s: %s overlaps %s (a written operand shares no element with another; interleaved address "
                         "ranges need equal row strides)", who, X.name, Y.name);
        }
    }
    return TRLX_OK;
}

static FaArgs fa_args(const TrlxT5FfActArgs* a, unsigned nct) {
    FaArgs k = {};
    k.u = a->u, k.v = a->v, k.dy = a->dy, k.out = a->out, k.du = a->du, k.dv = a->dv;
    k.ld_u = a->ld_u, k.ld_v = a->ld_v, k.ld_out = a->ld_out, k.ld_dy = a->ld_dy, k.ld_du = a->ld_du, k.ld_dv = a->ld_dv;
    k.N = a->N, k.F = a->F, k.nct = nct;
    return k;
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_ff_act_geometry(int* vec_bf16, int* vec_f32, int* cols_per_block, int* rows_per_block) {
    if (vec_bf16) *vec_bf16 = BF16T::kEPV;
    if (vec_f32) *vec_f32 = F32T::kEPV;
    if (cols_per_block) *cols_per_block = kFaCols;
    if (rows_per_block) *rows_per_block = kFaRows;
    return TRLX_OK;
}

extern "C" int trlx_t5_ff_act_fwd(const TrlxT5FfActArgs* a, void* stream) {
    const char* who = "t5 ff act fwd";
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->u && a->out, TRLX_ERR_ARG, "%s: NULL u / out", who);
    FaOp ops[3];
    int n = 0;
    ops[n++] = {"u", a->u, a->ld_u, false, 0};
    if (a->v) ops[n++] = {"v", a->v, a->ld_v, false, 0};
    ops[n++] = {"out", a->out, a->ld_out, true, 0};
    unsigned nct;
    bool vec, launch;
    const int rc = fa_check(who, a, ops, n, &nct, &vec, &launch);
    if (rc != TRLX_OK || !launch) return rc;
    const bool bf = a->dtype == TRLX_BF16, gated = a->v != nullptr;
    const fa_kernel_t fn = bf ? (vec ? fa_pick_fwd<BF16T, true>(a->act, gated) : fa_pick_fwd<BF16T, false>(a->act, gated))
                              : (vec ? fa_pick_fwd<F32T, true>(a->act, gated) : fa_pick_fwd<F32T, false>(a->act, gated));
    const unsigned grid = unsigned((a->N + kFaRows - 1) / kFaRows) * nct;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kFaThreads), 0, (hipStream_t)stream, fa_args(a, nct));
    return check_launch("k_t5_ff_act_fwd");
}

extern "C" int trlx_t5_ff_act_bwd(const TrlxT5FfActArgs* a, void* stream) {
    const char* who = "t5 ff act bwd";
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->u && a->dy, TRLX_ERR_ARG, "%s: NULL u / dy", who);
    TRLX_REQUIRE(a->du || a->dv, TRLX_ERR_ARG, "%s: neither du nor dv asked for", who);
    TRLX_REQUIRE(!a->dv || a->v, TRLX_ERR_ARG, "%s: dv asked for with no v", who);
    const bool read_v = a->v && a->du;
    FaOp ops[5];
    int n = 0;
    ops[n++] = {"dy", a->dy, a->ld_dy, false, 0};
    ops[n++] = {"u", a->u, a->ld_u, false, 0};
    if (a->v) ops[n++] = {"v", a->v, a->ld_v, false, 0};
    if (a->du) ops[n++] = {"du", a->du, a->ld_du, true, 0};
    if (a->dv) ops[n++] = {"dv", a->dv, a->ld_dv, true, 0};
    unsigned nct;
    bool vec, launch;
    const int rc = fa_check(who, a, ops, n, &nct, &vec, &launch);
    if (rc != TRLX_OK || !launch) return rc;
    const int mode = !a->v ? kFaDu : (a->du && a->dv) ? kFaDuDv : read_v ? kFaGatedDu : kFaDv;
    const bool bf = a->dtype == TRLX_BF16;
    const fa_kernel_t fn = bf ? (vec ? fa_pick_bwd<BF16T, true>(a->act, mode) : fa_pick_bwd<BF16T, false>(a->act, mode))
                              : (vec ? fa_pick_bwd<F32T, true>(a->act, mode) : fa_pick_bwd<F32T, false>(a->act, mode));
    const unsigned grid = unsigned((a->N + kFaRows - 1) / kFaRows) * nct;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kFaThreads), 0, (hipStream_t)stream, fa_args(a, nct));
    return check_launch("k_t5_ff_act_bwd");
}
