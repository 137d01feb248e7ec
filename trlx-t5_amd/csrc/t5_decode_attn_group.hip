// The decode cross-attention over encoder keys / values that the G samples of a prompt share: one
// launch, one workgroup per (prompt, head, tile of up to GT queries).  See trlx_t5_decode_attn_group
// in trlx_t5_amd.h.  Row b = p * G + g of q / out / live is sample g of prompt p, the order of
// repeat_interleave(G, dim = 0).
//
// The kernel is t5_group_body (t5_decode_attn_group.h) over all S keys; the split entry
// (t5_decode_attn_split.hip) runs the same body over ranges of them.  This unit also holds the
// argument checks that the grouped, the MFMA and the split entries share (t5_decode_group_check.h).
#include "t5_decode_attn_group.h"

namespace trlx {

template <class DT, int DKV, bool MASKED, bool LIVE, int GT>
__global__ __launch_bounds__(kT5RowThreads) void k_t5_decode_attn_group(const T5AttnGroupArgs a) {
    t5_group_body<DT, DKV, MASKED, LIVE, GT, false>(a);
}

struct T5GroupKernel {
    template <class DT, int DKV, bool MASKED, bool LIVE, int GT>
    static auto get() {
        return k_t5_decode_attn_group<DT, DKV, MASKED, LIVE, GT>;
    }
};

// The built query tiles are 1, 2, 4 and 8.  kT5GDefaultTile is the largest the entry takes unless
// trlx_t5_decode_attn_group_tile says otherwise.  A G below it takes the smallest built tile that
// holds G, so at T5-base, P 64 x G 4, S 512 a cap of 4 and a cap of 8 launch the same GT 4 kernel
// (33.5 and 32.7 us, the spreads one inside the other); at G 8, where they differ, two GT 4 tiles
// take 32.2 us and one GT 8 tile 44.1 us (profiles/t5_cross_group_bench.json).
constexpr int kT5GDefaultTile = 4;
static TuneKnob g_group_tile = {0};   // 0: kT5GDefaultTile

int t5_group_tile_cap() { return g_group_tile ? int(g_group_tile) : kT5GDefaultTile; }

int t5_group_tile(int64_t G) {
    const int cap = t5_group_tile_cap();
    int gt = 1;
    while (gt < cap && gt < G) gt *= 2;
    return gt;
}

int t5_group_check(const TrlxT5DecodeAttnGroupArgs* a, const char* who, bool f32_ok, bool rows_by_heads, int tile,
                   T5GroupChecked* c, int64_t d_only) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->dtype == TRLX_BF16 || (f32_ok && a->dtype == TRLX_F32), TRLX_ERR_ARG, "%s: dtype %d (%s only)", who,
                 a->dtype, f32_ok ? "bf16 and fp32" : "bf16");
    if (d_only)
        TRLX_REQUIRE(a->d_kv == d_only, TRLX_ERR_ARG, "%s: d_kv %lld (%lld only)", who, (long long)a->d_kv, (long long)d_only);
    else
        TRLX_REQUIRE(a->d_kv == 64 || a->d_kv == 128, TRLX_ERR_ARG, "%s: d_kv %lld (64 and 128 only)", who, (long long)a->d_kv);
    TRLX_REQUIRE(a->P >= 1 && a->G >= 1 && a->n_heads >= 1 && a->S >= 1, TRLX_ERR_ARG,
                 "%s: P %lld, G %lld, heads %lld, S %lld (all >= 1)", who, (long long)a->P, (long long)a->G,
                 (long long)a->n_heads, (long long)a->S);
    // the grid is (P * heads, ceil(G / tile)[, X]); rows, heads and keys are 32-bit in the kernels
    TRLX_REQUIRE(a->P <= 0x7fffffffLL && a->G <= 0x7fffffffLL && a->n_heads <= 0x7fffffffLL / 128 &&
                     a->S <= 0x7fffffffLL / 128 && a->P * a->n_heads <= 0x7fffffffLL && a->P * a->G <= 0x7fffffffLL &&
                     (!rows_by_heads || a->P * a->G * a->n_heads <= 0x7fffffffLL),
                 TRLX_ERR_ARG, "%s: P %lld, G %lld, heads %lld, S %lld overflow the grid", who, (long long)a->P,
                 (long long)a->G, (long long)a->n_heads, (long long)a->S);
    TRLX_REQUIRE(a->q && a->k && a->v && a->out, TRLX_ERR_ARG, "%s: NULL q / K / V / out", who);
    const int64_t inner = a->n_heads * a->d_kv;
    const int64_t epv = a->dtype == TRLX_BF16 ? 8 : 4;
    c->ldq = a->P * a->G == 1 ? inner : a->ldq;   // a single row has no stride to speak of
    TRLX_REQUIRE(c->ldq >= inner && c->ldq % epv == 0, TRLX_ERR_ARG,
                 "%s: q row stride %lld (>= heads * d_kv = %lld, whole 16-byte vectors)", who, (long long)c->ldq,
                 (long long)inner);
    // a dimension of size 1 has no stride to speak of
    const int64_t st[6] = {a->P > 1 ? a->k_stride_p : 0, a->n_heads > 1 ? a->k_stride_h : 0, a->S > 1 ? a->k_stride_s : 0,
                           a->P > 1 ? a->v_stride_p : 0, a->n_heads > 1 ? a->v_stride_h : 0, a->S > 1 ? a->v_stride_s : 0};
    for (int i = 0; i < 6; ++i) {
        TRLX_REQUIRE(st[i] >= 0 && st[i] % epv == 0, TRLX_ERR_ARG, "%s: stride %lld (non-negative, whole 16-byte vectors)",
                     who, (long long)st[i]);
        c->st[i] = st[i];
    }
    TRLX_REQUIRE((a->S == 1 || (st[2] >= a->d_kv && st[5] >= a->d_kv)) &&
                     (a->n_heads == 1 || (st[1] >= a->d_kv && st[4] >= a->d_kv)),
                 TRLX_ERR_ARG, "%s: key and head strides must be at least d_kv", who);
    auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    TRLX_REQUIRE(!mis(a->q, 15) && !mis(a->k, 15) && !mis(a->v, 15) && !mis(a->out, 15), TRLX_ERR_ARG,
                 "%s: q, K, V and out must be 16-byte aligned", who);
    TRLX_REQUIRE(!mis(a->key_mask, 7) && !mis(a->live, 7), TRLX_ERR_ARG, "%s: key_mask and live must be 8-byte aligned", who);
    c->gt = tile ? tile : t5_group_tile(a->G);
    c->tiles = (a->G + c->gt - 1) / c->gt;
    TRLX_REQUIRE(c->tiles <= 65535, TRLX_ERR_ARG, "%s: G %lld gives %lld query tiles (at most 65535)", who, (long long)a->G,
                 (long long)c->tiles);
    return TRLX_OK;
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_decode_attn_group_tile(int64_t tile) {
    TRLX_REQUIRE(tile == 0 || tile == 1 || tile == 2 || tile == 4 || tile == 8, TRLX_ERR_ARG,
                 "t5 grouped decode attention: query tile %lld (0 = default, 1, 2, 4 or 8)", (long long)tile);
    g_group_tile = int(tile);
    return TRLX_OK;
}

extern "C" int trlx_t5_decode_attn_group(const TrlxT5DecodeAttnGroupArgs* a, void* stream) {
    T5GroupChecked c;
    const int rc = t5_group_check(a, "t5 grouped decode attention", true, false, 0, &c);
    if (rc) return rc;
    T5AttnGroupArgs k = {};
    t5_group_fill(k, a, c);
    hipLaunchKernelGGL(t5_group_pick<T5GroupKernel>(a->dtype, a->d_kv, c.gt, a->key_mask != nullptr, a->live != nullptr),
                       dim3(unsigned(a->P * a->n_heads), unsigned(c.tiles)), dim3(kT5RowThreads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn_group");
}
