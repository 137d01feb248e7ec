// Device-resident ILQL rollout store: the ragged collate and the device half of
// make_experience — replaces OfflineOrchestrator.make_experience's per-sample host tensors
// (offline_orchestrator.py:17-74), ILQLRolloutStorage's pad_sequence collate
// (offline_pipeline.py:87-112) and to_device(batch) (accelerate_ilql_model.py:58-68).
//
// The store is the whole static offline dataset with widely varying sample lengths and five
// int64 fields of six, so it is ragged, not the PPO store's padded [capacity, W] buffers: six
// flat buffers in three offset families (L: input_ids / attention_mask, S: states_ixs / dones,
// A: actions_ixs / rewards), each family with an int64 prefix-sum vector off[N + 1].
//   k_ilql_collate       out_f[j, c] = c < len(idx[j]) ? flat_f[off[idx[j]] + c] : 0 — pads while
//                        it gathers, one launch per training batch.
//   k_ilql_build_fields  the five derived fields of every sample from (offsets, prompt length,
//                        raw reward, the rewards' moments record), one launch per dataset.
// Both: grid.y = field, one wave per (row, field), lanes striding over the row as in
// k_rows_copy.  Pure data movement, launch / latency bound.
#include "common.h"

namespace trlx {

constexpr int kIlqlFields = 6;  // ILQLBatch order: input_ids, attention_mask, rewards, states_ixs, actions_ixs, dones
constexpr int kIlqlRewards = 2;  // the one fp32 field
constexpr int kStoreThreads = 256;
constexpr int kStoreRowsPerBlock = kStoreThreads / kWave;

struct IlqlCollateArgs {
    const void* flat[kIlqlFields];
    const int64_t* off[kIlqlFields];  // the field's family offsets
    void* out[kIlqlFields];
    int64_t ld[kIlqlFields], W[kIlqlFields];
    const int64_t* idx;
    int64_t n, N;
};

template <typename E>
__device__ __forceinline__ void collate_row(const void* flat, int64_t beg, int64_t len, void* out, int64_t W,
                                            int lane) {
    const E* s = reinterpret_cast<const E*>(flat) + beg;
    E* d = reinterpret_cast<E*>(out);
    for (int64_t c = lane; c < W; c += kWave) d[c] = c < len ? s[c] : E(0);
}

__global__ __launch_bounds__(kStoreThreads) void k_ilql_collate(IlqlCollateArgs a) {
    const int64_t j = int64_t(blockIdx.x) * kStoreRowsPerBlock + threadIdx.x / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    if (j >= a.n) return;
    const int f = blockIdx.y;
    const int64_t i = a.idx[j];
    int64_t beg = 0, len = 0;
    if (i >= 0 && i < a.N) {  // a sample number outside the store gives a pad row, never a read
        beg = a.off[f][i];
        len = a.off[f][i + 1] - beg;
    }
    if (f == kIlqlRewards)  // a rewards row is only 4-byte aligned (off_A may be odd)
        collate_row<float>(a.flat[f], beg, len, static_cast<float*>(a.out[f]) + j * a.ld[f], a.W[f], lane);
    else
        collate_row<int64_t>(a.flat[f], beg, len, static_cast<int64_t*>(a.out[f]) + j * a.ld[f], a.W[f], lane);
}

// grid.y: 0 attention_mask, 1 states_ixs, 2 actions_ixs, 3 dones, 4 rewards.
enum { kBuildMask = 0, kBuildStates, kBuildActions, kBuildDones, kBuildRewards, kBuildFields };

struct IlqlBuildArgs {
    const int64_t *off_L, *off_S, *off_A, *prompt_len;
    const float* rewards;
    const double* stats;
    int64_t N, total_L, total_S, total_A;
    int64_t *attention_mask, *states_ixs, *actions_ixs, *dones;
    float* out_rewards;
};

__global__ __launch_bounds__(kStoreThreads) void k_ilql_build_fields(IlqlBuildArgs a) {
    const int64_t i = int64_t(blockIdx.x) * kStoreRowsPerBlock + threadIdx.x / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    if (i >= a.N) return;
    const int f = blockIdx.y;
    const int64_t* off = f == kBuildMask ? a.off_L : (f == kBuildStates || f == kBuildDones) ? a.off_S : a.off_A;
    const int64_t total = f == kBuildMask ? a.total_L : (f == kBuildStates || f == kBuildDones) ? a.total_S : a.total_A;
    const int64_t beg = off[i];
    int64_t len = off[i + 1] - beg;
    if (beg < 0) return;
    if (len > total - beg) len = total - beg;  // never past the buffer, whatever the offsets hold
    const int64_t first = a.prompt_len[i] - 1;  // index of the last prompt token
    if (f == kBuildMask) {
        for (int64_t c = lane; c < len; c += kWave) a.attention_mask[beg + c] = 1;
    } else if (f == kBuildStates) {
        for (int64_t c = lane; c < len; c += kWave) a.states_ixs[beg + c] = first + c;
    } else if (f == kBuildActions) {
        for (int64_t c = lane; c < len; c += kWave) a.actions_ixs[beg + c] = first + c;
    } else if (f == kBuildDones) {
        for (int64_t c = lane; c < len; c += kWave) a.dones[beg + c] = c < len - 1 ? 1 : 0;
    } else {
        // G = (r - mean) / (std + 1e-30), unbiased std, from the record {sum, sumsq, count}
        // (the formula of k_whiten_apply); count 1 gives 0 / 0 = NaN as torch's std() does.
        const double cnt = a.stats[2];
        const double mean = a.stats[0] / cnt;
        double m2 = a.stats[1] - a.stats[0] * mean;
        if (m2 < 0) m2 = 0;
        const double sd = sqrt(m2 / (cnt - 1.0));
        const float G = float((double(a.rewards[i]) - mean) / (sd + 1e-30));
        for (int64_t c = lane; c < len; c += kWave) a.out_rewards[beg + c] = c == len - 1 ? G : 0.0f;
    }
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_ilql_collate(const int64_t* input_ids, const int64_t* attention_mask, const float* rewards,
                                 const int64_t* states_ixs, const int64_t* actions_ixs, const int64_t* dones,
                                 const int64_t* off_L, const int64_t* off_S, const int64_t* off_A, int64_t N,
                                 const int64_t* idx, int64_t n, int64_t WL, int64_t WS, int64_t WA,
                                 int64_t* out_input_ids, int64_t ld_input_ids, int64_t* out_attention_mask,
                                 int64_t ld_attention_mask, float* out_rewards, int64_t ld_rewards,
                                 int64_t* out_states_ixs, int64_t ld_states_ixs, int64_t* out_actions_ixs,
                                 int64_t ld_actions_ixs, int64_t* out_dones, int64_t ld_dones, void* stream) {
    TRLX_REQUIRE(N >= 0 && n >= 0 && n < (int64_t(1) << 31) * kStoreRowsPerBlock, TRLX_ERR_SHAPE,
                 "ilql_collate: bad sizes N=%lld n=%lld", (long long)N, (long long)n);
    TRLX_REQUIRE(WL >= 0 && WS >= 0 && WA >= 0, TRLX_ERR_SHAPE, "ilql_collate: negative width WL=%lld WS=%lld WA=%lld",
                 (long long)WL, (long long)WS, (long long)WA);
    IlqlCollateArgs a = {};
    const void* flat[kIlqlFields] = {input_ids, attention_mask, rewards, states_ixs, actions_ixs, dones};
    const int64_t* off[kIlqlFields] = {off_L, off_L, off_A, off_S, off_A, off_S};
    void* out[kIlqlFields] = {out_input_ids, out_attention_mask, out_rewards, out_states_ixs, out_actions_ixs, out_dones};
    const int64_t ld[kIlqlFields] = {ld_input_ids, ld_attention_mask, ld_rewards, ld_states_ixs, ld_actions_ixs, ld_dones};
    const int64_t W[kIlqlFields] = {WL, WL, WA, WS, WA, WS};
    for (int f = 0; f < kIlqlFields; ++f)
        TRLX_REQUIRE(ld[f] >= W[f], TRLX_ERR_STRIDE, "ilql_collate: field %d row stride %lld < width %lld", f,
                     (long long)ld[f], (long long)W[f]);
    if (n == 0) return TRLX_OK;
    TRLX_REQUIRE(idx && off_L && off_S && off_A, TRLX_ERR_ARG, "NULL idx / offsets to trlx_ilql_collate");
    for (int f = 0; f < kIlqlFields; ++f) {
        TRLX_REQUIRE(flat[f], TRLX_ERR_ARG, "ilql_collate: NULL store field %d", f);
        TRLX_REQUIRE(out[f] || W[f] == 0, TRLX_ERR_ARG, "ilql_collate: NULL output field %d", f);
        a.flat[f] = flat[f];
        a.off[f] = off[f];
        a.out[f] = out[f];
        a.ld[f] = ld[f];
        a.W[f] = W[f];
    }
    a.idx = idx;
    a.n = n;
    a.N = N;
    const dim3 grid(unsigned((n + kStoreRowsPerBlock - 1) / kStoreRowsPerBlock), unsigned(kIlqlFields));
    hipLaunchKernelGGL(k_ilql_collate, grid, dim3(kStoreThreads), 0, (hipStream_t)stream, a);
    return check_launch("k_ilql_collate");
}

extern "C" int trlx_ilql_build_fields(const int64_t* off_L, const int64_t* off_S, const int64_t* off_A,
                                      const int64_t* prompt_len, const float* rewards, const double* stats,
                                      int64_t N, int64_t total_L, int64_t total_S, int64_t total_A,
                                      int64_t* attention_mask, int64_t* states_ixs, int64_t* actions_ixs,
                                      int64_t* dones, float* out_rewards, void* stream) {
    TRLX_REQUIRE(N >= 0 && N < (int64_t(1) << 31) * kStoreRowsPerBlock && total_L >= 0 && total_S >= 0 && total_A >= 0,
                 TRLX_ERR_SHAPE, "ilql_build_fields: bad sizes N=%lld totals %lld %lld %lld", (long long)N,
                 (long long)total_L, (long long)total_S, (long long)total_A);
    if (N == 0) return TRLX_OK;
    TRLX_REQUIRE(off_L && off_S && off_A && prompt_len && rewards && stats, TRLX_ERR_ARG,
                 "NULL input to trlx_ilql_build_fields");
    TRLX_REQUIRE(attention_mask && states_ixs && actions_ixs && dones && out_rewards, TRLX_ERR_ARG,
                 "NULL output to trlx_ilql_build_fields");
    IlqlBuildArgs a = {off_L, off_S, off_A, prompt_len, rewards, stats, N, total_L, total_S, total_A,
                       attention_mask, states_ixs, actions_ixs, dones, out_rewards};
    const dim3 grid(unsigned((N + kStoreRowsPerBlock - 1) / kStoreRowsPerBlock), unsigned(kBuildFields));
    hipLaunchKernelGGL(k_ilql_build_fields, grid, dim3(kStoreThreads), 0, (hipStream_t)stream, a);
    return check_launch("k_ilql_build_fields");
}
