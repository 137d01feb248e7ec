// The decode cross-attention with the encoder keys of a (row, head) split across workgroups: two
// launches in stream order, no atomics, no counters, no spinning.  See trlx_t5_decode_attn_split in
// trlx_t5_amd.h.  The interface is the grouped entry's (t5_decode_attn_group.hip): P prompts, G
// samples a prompt, row b = p * G + g, K / V through element strides, key_mask per prompt, live per
// row.  G = 1 is the plain cross-attention.
//
// k_t5_decode_attn_split_part, grid (P * nH, tiles, X): workgroup (ph, tile, x) is
// k_t5_decode_attn_group restricted to the keys [x * C, min(S, (x + 1) * C)): the same body,
// t5_group_body of t5_decode_attn_group.h, with SPLIT set.  C is a multiple of NG, so key j is walked
// by group j % NG as in the unsplit kernel.  The workgroup stops before the division: per live query
// it writes the unnormalised state (M, L, o[d_kv]) in fp32 to the workspace, M = -inf and L = 0 when
// the range held no live key.  A tile whose queries are all dead writes nothing and forms no
// address into q, K, V or the mask; a dead query of a live tile writes nothing either.
//
// k_t5_decode_attn_split_merge: one thread per two outputs of a (row, head) reads the row's states
// in split order, M = max M_x, and for every x with M_x != -inf  w = expf(M_x - M),
// L = fmaf(L_x, w, L), o = fmaf(o_x, w, o); then o / L (zeros when no key was live) and one rounding.
// A dead row gets zeros and its states are not read.
//
// The result depends on X and on nothing else: not on P, the strides or the query tile.  It is not
// the unsplit kernel's bits for X > 1: the unsplit merge weighs all NG groups against one maximum,
// here the groups of a range are weighed against the range's maximum and the ranges against the
// global one, so the roundings of expf and of the sums fall differently.  With one range holding
// every live key the weights of the merge are expf(0) = 1 and the bits are the unsplit kernel's.
//
// Kernels in a translation unit of their own; the part kernel's arithmetic is the grouped kernel's
// because it is the same text, and the merge kernel finishes with t5_decode_row.h's division and store.
#include "t5_decode_attn_group.h"

namespace trlx {

constexpr int kT5SMaxSplits = 8;  // the largest X the entry takes

// T5AttnGroupArgs's fields under their names, which t5_group_body reads, and the split's own, in the
// order the kernels have always taken them.
struct T5AttnSplitArgs {
    const void* q;
    const void* k;
    const void* v;
    const int64_t* mask;    // [P, S] or NULL (MASKED = false)
    const int64_t* live;    // [P * G] or NULL (LIVE = false)
    float* ws;              // [P * G, nH, X, DKV + 2]: M, L, o[DKV]
    void* out;
    int64_t ldq;
    int64_t k_sp, k_sh, k_ss, v_sp, v_sh, v_ss;   // element strides over (p, h, s)
    int nH, G, S;
    int C, X;               // keys a range, ranges launched
    int rows;               // P * G
};

// blockIdx.x = p * nH + h, blockIdx.y = the query tile, blockIdx.z = the key range.
template <class DT, int DKV, bool MASKED, bool LIVE, int GT>
__global__ __launch_bounds__(kT5RowThreads) void k_t5_decode_attn_split_part(const T5AttnSplitArgs a) {
    t5_group_body<DT, DKV, MASKED, LIVE, GT, true>(a);
}

// Thread t of the grid: outputs d, d + 1 of (row, head) = t / (DKV / 2).
template <class DT, int DKV, bool LIVE>
__global__ __launch_bounds__(kT5RowThreads) void k_t5_decode_attn_split_merge(const T5AttnSplitArgs a) {
    typedef typename DT::elem_t E;
    constexpr int REC = DKV + 2;
    const int64_t t = int64_t(blockIdx.x) * kT5RowThreads + threadIdx.x;
    const int64_t bh = t / (DKV / 2);
    if (bh >= int64_t(a.rows) * a.nH) return;
    const int d = 2 * int(t - bh * (DKV / 2));
    float o0 = 0.f, o1 = 0.f;
    bool dead = false;
    if constexpr (LIVE) dead = a.live[bh / a.nH] == 0;
    if (!dead) {
        const float* rec = a.ws + bh * a.X * REC;
        float M = rec[0];
        for (int x = 1; x < a.X; ++x) M = fmaxf(M, rec[x * REC]);
        float L = 0.f;
        for (int x = 0; x < a.X; ++x) {
            const float2 ml = *reinterpret_cast<const float2*>(rec + x * REC);
            if (ml.x == -INFINITY) continue;   // a range that held no live key
            const float2 o = *reinterpret_cast<const float2*>(rec + x * REC + 2 + d);
            const float w = expf(ml.x - M);
            L = fmaf(ml.y, w, L);
            o0 = fmaf(o.x, w, o0);
            o1 = fmaf(o.y, w, o1);
        }
        t5_row_divide(L, o0, o1);
    }
    t5_store_pair<E>(a.out, bh * DKV + d, o0, o1);
}

typedef void (*t5_split_kernel_t)(const T5AttnSplitArgs);
struct T5SplitPartKernel {
    template <class DT, int DKV, bool MASKED, bool LIVE, int GT>
    static auto get() {
        return k_t5_decode_attn_split_part<DT, DKV, MASKED, LIVE, GT>;
    }
};
template <class DT, int DKV>
static t5_split_kernel_t t5_split_pick_merge_live(bool live) {
    return live ? k_t5_decode_attn_split_merge<DT, DKV, true> : k_t5_decode_attn_split_merge<DT, DKV, false>;
}
static t5_split_kernel_t t5_split_pick_merge(int dtype, int64_t d_kv, bool live) {
    if (dtype == TRLX_BF16)
        return d_kv == 64 ? t5_split_pick_merge_live<BF16T, 64>(live) : t5_split_pick_merge_live<BF16T, 128>(live);
    return d_kv == 64 ? t5_split_pick_merge_live<F32T, 64>(live) : t5_split_pick_merge_live<F32T, 128>(live);
}

// NG of the kernels' geometry: 4 waves * (64 lanes / (d_kv / elements a 16-byte vector)).
static int t5_split_groups(int dtype, int64_t d_kv) {
    const int epv = dtype == TRLX_BF16 ? 8 : 4;
    return kT5RowWaves * (kWave / int(d_kv / epv));
}
// C: ceil(S / X) rounded up to a multiple of NG.
static int64_t t5_split_range(int64_t S, int64_t X, int ng) {
    const int64_t c = (S + X - 1) / X;
    return (c + ng - 1) / ng * ng;
}
static bool t5_split_geometry_ok(int dtype, int64_t d_kv) {
    return (dtype == TRLX_BF16 || dtype == TRLX_F32) && (d_kv == 64 || d_kv == 128);
}

}  // namespace trlx

using namespace trlx;

extern "C" int64_t trlx_t5_decode_attn_split_workspace_bytes(int64_t rows, int64_t n_heads, int64_t d_kv, int64_t splits) {
    if (rows < 1 || n_heads < 1 || (d_kv != 64 && d_kv != 128) || splits < 1 || splits > kT5SMaxSplits) return 0;
    if (rows > 0x7fffffffLL || n_heads > 0x7fffffffLL / 128 || rows * n_heads > 0x7fffffffLL) return 0;
    return rows * n_heads * splits * (d_kv + 2) * int64_t(sizeof(float));
}

extern "C" int trlx_t5_decode_attn_split_geometry(int dtype, int64_t d_kv, int64_t S, int64_t splits,
                                                  TrlxT5DecodeAttnSplitGeometry* g) {
    TRLX_REQUIRE(g, TRLX_ERR_ARG, "t5 split decode attention geometry: NULL result");
    *g = TrlxT5DecodeAttnSplitGeometry{};
    TRLX_REQUIRE(t5_split_geometry_ok(dtype, d_kv), TRLX_ERR_ARG,
                 "t5 split decode attention geometry: dtype %d, d_kv %lld (bf16 / fp32, 64 / 128)", dtype, (long long)d_kv);
    TRLX_REQUIRE(S >= 1 && S <= 0x7fffffffLL / 128, TRLX_ERR_ARG, "t5 split decode attention geometry: S %lld", (long long)S);
    TRLX_REQUIRE(splits >= 1 && splits <= kT5SMaxSplits, TRLX_ERR_ARG,
                 "t5 split decode attention geometry: splits %lld (1 to %d)", (long long)splits, kT5SMaxSplits);
    g->NG = t5_split_groups(dtype, d_kv);
    g->C = t5_split_range(S, splits, int(g->NG));
    g->ranges = (S + g->C - 1) / g->C;
    g->tile = t5_group_tile_cap();
    g->max_splits = kT5SMaxSplits;
    return TRLX_OK;
}

// The X taken for splits == 0.  A pure function of the shape: not of live, not of the device, not
// of the tile knob (W below counts tiles of the default cap).  Set from
// profiles/t5_cross_split_bench.json ("Encoder keys split across workgroups"):
// per shape class the X whose median inside a replayed graph beat the best existing route by more
// than that route's own min-max spread, 1 where none did.  W = the unsplit grid, R = the keys a
// group walks.
//   W > 256               1   measured at W 768 (P 64 x G 4, P 32 x G 8), 3072 (B 256) and 4096: every X loses or ties
//   R < 32                1   measured at R 16 (T5-base S 512, W 96 and W 24): a tie with the plain call, a loss to it
//   W <= 64               8   W 24, R 64 (P 2 x G 4, S 2048): 22.2 us against 33.3 (X 4: 25.1)
//   W <= 128              4   W 96, R 64 (T5-base B 8, S 2048): 18.9 us against 32.4 (X 2: 22.9, X 8: 21.3)
//   W <= 256              2   W 256, R 32 and R 128 (nH 32, d 128, B 8): 18.3 against 21.1, 55.4 against 81.3 (X 4: 20.2, 57.1)
// and X halved until a range keeps 8 keys a group, the shortest range that was measured to win.
// fp32 was not measured: 1.
extern "C" int trlx_t5_decode_attn_split_plan(int dtype, int64_t P, int64_t G, int64_t n_heads, int64_t d_kv, int64_t S) {
    if (!t5_split_geometry_ok(dtype, d_kv) || P < 1 || G < 1 || n_heads < 1 || S < 1) return 1;
    if (dtype != TRLX_BF16) return 1;
    int64_t tile = 1;   // the default cap's tile, whatever the knob says
    while (tile < 4 && tile < G) tile *= 2;
    if (P > 256 || n_heads > 256 || G > 1024) return 1;
    const int64_t W = P * n_heads * ((G + tile - 1) / tile);
    if (W > 256) return 1;
    const int ng = t5_split_groups(dtype, d_kv);
    const int64_t R = (S + ng - 1) / ng;
    if (R < 32) return 1;
    int X = W <= 64 ? 8 : W <= 128 ? 4 : 2;
    while (X > 1 && R / X < 8) X /= 2;
    return X;
}

extern "C" int trlx_t5_decode_attn_split(const TrlxT5DecodeAttnGroupArgs* a, int64_t splits, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
    T5GroupChecked c;
    const int rc0 = t5_group_check(a, "t5 split decode attention", true, true, 0, &c);
    if (rc0) return rc0;
    TRLX_REQUIRE(splits >= 0 && splits <= kT5SMaxSplits, TRLX_ERR_ARG,
                 "t5 split decode attention: splits %lld (0 = the plan, 1 to %d)", (long long)splits, kT5SMaxSplits);
    const int64_t X = splits ? splits : trlx_t5_decode_attn_split_plan(a->dtype, a->P, a->G, a->n_heads, a->d_kv, a->S);
    const int64_t need = trlx_t5_decode_attn_split_workspace_bytes(a->P * a->G, a->n_heads, a->d_kv, X);
    TRLX_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 && workspace_bytes >= need, TRLX_ERR_ARG,
                 "t5 split decode attention: workspace %p of %lld bytes (16-byte aligned, at least %lld bytes for %lld splits)",
                 workspace, (long long)workspace_bytes, (long long)need, (long long)X);
    if (X == 1) return trlx_t5_decode_attn_group(a, stream);   // one range: the unsplit kernel, one launch

    const int ng = t5_split_groups(a->dtype, a->d_kv);
    const int64_t C = t5_split_range(a->S, X, ng);
    const int64_t ranges = (a->S + C - 1) / C;   // the non-empty ones, <= X
    T5AttnSplitArgs k = {};
    t5_group_fill(k, a, c);
    k.ws = static_cast<float*>(workspace);
    k.C = int(C);
    k.X = int(ranges);
    k.rows = int(a->P * a->G);
    hipLaunchKernelGGL(t5_group_pick<T5SplitPartKernel>(a->dtype, a->d_kv, c.gt, a->key_mask != nullptr, a->live != nullptr),
                       dim3(unsigned(a->P * a->n_heads), unsigned(c.tiles), unsigned(ranges)), dim3(kT5RowThreads), 0,
                       (hipStream_t)stream, k);
    const int rc = check_launch("k_t5_decode_attn_split_part");
    if (rc != TRLX_OK) return rc;
    const int64_t threads = a->P * a->G * a->n_heads * (a->d_kv / 2);
    hipLaunchKernelGGL(t5_split_pick_merge(a->dtype, a->d_kv, a->live != nullptr),
                       dim3(unsigned((threads + kT5RowThreads - 1) / kT5RowThreads)), dim3(kT5RowThreads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn_split_merge");
}
