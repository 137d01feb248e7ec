// Vocab-axis sampling step of PPO rollout generation, one workgroup per row: the logits
// processors and the draw of HF generate's sample path (transformers 4.21, as called by
// ppo_orchestrator.py:76 / ppo_models.py:620-622 with PPOConfig.gen_kwargs), per row b:
//
//   x      = logits[b, :] in fp32;  x[eos] = -inf while cur_len < min_length
//   keep   = x >= k-th largest x                       (top-k; ties at the threshold kept)
//   w      = exp((x - max x) / T) over the kept,  W = sum w
//   keep  &= mass{x' > x} <= top_p * W  or  x among the min_tokens_to_keep largest
//            (top-p, the 4.21 rule: the token that crosses top_p stays; every tie at the
//            nucleus boundary is kept, where HF keeps whichever its sort placed first)
//   token  = inverse CDF of w over the kept at u[b], vocab-index order
//   token  = unfinished ? token : pad;  unfinished &= token != eos
//   logprob = log_softmax(logits[b, :])[token]          (the unmodified row)
//
// Filtering is defined on the order of x (division by T > 0 is monotone).  The row is held
// in VGPRs as in ilql_sample.hip (16-B non-temporal buffer loads on the rows' 256-B line
// shift).  Nothing is sorted: the k-th largest value and the nucleus threshold are each the
// result of a search over order-preserving uint32 keys.  Fast path: a candidate list in LDS
// (the values above a lower bound of the n-th largest, n = k or a seed of 128 for top-p
// alone) is ranked by one thread per candidate.  Rows that defeat it (ties, k above the
// thread count, a nucleus wider than the list) take 32-step block-wide bisections: on counts
// for top-k, on mass for top-p.  Block reductions run in a fixed order; the list's masses are
// summed in the order the waves filled it, and feed comparisons with top_p * W only.
#include "common.h"

#include <type_traits>

namespace trlx {

struct PpoSampleArgs {
    const void* logits;  // [B, V] rows of ld_logits
    int64_t ld_logits;
    int64_t V;
    float scale;         // log2(e) / temperature
    float top_p;
    int top_k;           // 0 = off, else already clamped to [min_keep, V]
    int min_keep;        // min_tokens_to_keep, <= V
    int suppress_eos;    // cur_len < min_length and eos given
    int64_t eos, pad;    // -1 = none
    const float* u;      // [B] uniforms in [0, 1)
    int64_t* out_ids;    // [B]
    float* out_lp;       // [B] log_softmax(logits)[id]
    float* out_min;      // [B] smallest kept logit
    int* out_cnt;        // [B] number of kept tokens
    int64_t* unfinished; // [B] in/out (0/1), NULL = all live
};

// The recording step (trlx_ppo_sample_record): the reference model's row of the same step and
// column t of the rollout's [B, T] buffers (row strides in elements).
struct PpoRecordArgs {
    const void* ref_logits;  // [B, V] rows of ld_ref, the dtype of the policy rows
    int64_t ld_ref;
    int64_t t;               // the column written
    int64_t* tokens;         // [B, T] int64
    int64_t ld_tokens;
    float* lp;               // [B, T] policy log-prob of the token
    int64_t ld_lp;
    float* ref_lp;           // [B, T] reference log-prob of the token
    int64_t ld_ref_lp;
    float* values;           // [B, T] or NULL
    int64_t ld_values;
    const void* v;           // [B] this step's values (v_dtype), NULL with values
    int v_dtype;
    int score_finished;      // finished rows: log-softmax of both rows at pad (else 0 and no read)
    int64_t* lengths;        // [B] or NULL: t + 1 where a live row returns eos
};

// order-preserving float -> uint32 (a larger float has a larger key) and back
__device__ __forceinline__ uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {  // NaN for keys no float maps to
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

constexpr int kPsCandCap = 512;   // candidate list in LDS, one per thread at most
constexpr int kPsSeed = 128;      // list size aimed at when top-p runs without top-k

struct PpoSampleRecArgs {
    PpoSampleArgs s;
    PpoRecordArgs r;
};
__device__ __forceinline__ const PpoSampleArgs& sample_args(const PpoSampleArgs& a) { return a; }
__device__ __forceinline__ const PpoSampleArgs& sample_args(const PpoSampleRecArgs& a) { return a.s; }
__device__ __forceinline__ PpoRecordArgs record_args(const PpoSampleArgs&) { return PpoRecordArgs{}; }
__device__ __forceinline__ PpoRecordArgs record_args(const PpoSampleRecArgs& a) { return a.r; }

// The processing step (trlx_ppo_sample_proc): HF's prefix-aware logits processors and the forced
// token.  The prefix of row b is seg0[b, 0:n0] followed by seg1[b, 0:n1] (row strides in elements).
struct PpoProcArgs {
    const int64_t* seg0;
    int64_t ld0;
    const int64_t* seg1;
    int64_t ld1;
    int n0, n1;
    const int64_t* bw_tok;   // bad words: flat tokens, sequence s = bw_tok[bw_off[s] .. bw_off[s + 1])
    const int64_t* bw_off;
    int n_bw;
    int ngram;               // 0 = off
    float rp;                // 1 = off
    int edits;               // any of the three on
    int64_t forced;          // -1 = none
};
struct PpoSampleProcArgs {
    PpoSampleArgs s;
    PpoRecordArgs r;         // r.ref_logits == NULL: no recording
    PpoProcArgs p;
};
__device__ __forceinline__ const PpoSampleArgs& sample_args(const PpoSampleProcArgs& a) { return a.s; }
__device__ __forceinline__ PpoRecordArgs record_args(const PpoSampleProcArgs& a) { return a.r; }
__device__ __forceinline__ PpoProcArgs proc_args(const PpoSampleArgs&) { return PpoProcArgs{}; }
__device__ __forceinline__ PpoProcArgs proc_args(const PpoSampleRecArgs&) { return PpoProcArgs{}; }
__device__ __forceinline__ PpoProcArgs proc_args(const PpoSampleProcArgs& a) { return a.p; }

// The device-clock step (trlx_ppo_sample_proc_dev): what the host entries decide per token from
// t and cur_len is decided by the kernel from the decode clock.  s.suppress_eos, r.t, p.n1 and
// p.forced of the argument block are not read.
struct PpoClockArgs {
    const int64_t* clock;    // {t, T, cur_len0, overrun, ...}
    int64_t T;               // the record buffers' columns
    int64_t min_length;
    int64_t forced_bos;      // -1 = none; at cur_len == 1
    int64_t forced_eos;      // -1 = none; at cur_len == max_length - 1, wins
    int64_t max_length;
    int64_t u_ld;            // 0: u is [B]; else row t of a [T, u_ld] table
};
struct PpoSampleRecClockArgs {
    PpoSampleArgs s;
    PpoRecordArgs r;
    PpoClockArgs c;
};
struct PpoSampleProcClockArgs {
    PpoSampleArgs s;
    PpoRecordArgs r;
    PpoProcArgs p;
    PpoClockArgs c;
};
__device__ __forceinline__ const PpoSampleArgs& sample_args(const PpoSampleRecClockArgs& a) { return a.s; }
__device__ __forceinline__ const PpoSampleArgs& sample_args(const PpoSampleProcClockArgs& a) { return a.s; }
__device__ __forceinline__ PpoRecordArgs record_args(const PpoSampleRecClockArgs& a) { return a.r; }
__device__ __forceinline__ PpoRecordArgs record_args(const PpoSampleProcClockArgs& a) { return a.r; }
__device__ __forceinline__ PpoProcArgs proc_args(const PpoSampleRecClockArgs&) { return PpoProcArgs{}; }
__device__ __forceinline__ PpoProcArgs proc_args(const PpoSampleProcClockArgs& a) { return a.p; }
template <bool REC, bool PROC, bool DEV = false>
using ppo_sample_args_t = std::conditional_t<
    DEV, std::conditional_t<PROC, PpoSampleProcClockArgs, PpoSampleRecClockArgs>,
    std::conditional_t<PROC, PpoSampleProcArgs, std::conditional_t<REC, PpoSampleRecArgs, PpoSampleArgs>>>;

// One row's step.  REC: the recording step — the reference row is reduced to per-wave
// (max, sum exp) pairs first, parked in LDS (nothing of it stays in registers while the
// policy row is held), and the thread that finds the token reads x_ref[token] beside x[token].
// The lambdas that the larger body would otherwise leave as calls are always_inline: a call
// takes the row's registers by reference, which puts the row in scratch.
// (One kernel template, not a shared device function called by two kernels: through such a
// wrapper hipcc 7.2 schedules the plain step differently — 89 -> 128 VGPRs + 52 B scratch at
// bf16 4 x 1024.  REC = false compiles to the kernel this file had before the recording step.)
//
// PROC: the processing step (an instantiation of its own, REC compiled in and switched by
// r.ref_logits at run time; PROC = false leaves the two kernels above as they were).  The
// prefix-aware processors are sparse edits of the row, gathered first as two bitmaps over V in
// LDS — "penalised" (repetition penalty) and "banned" (no-repeat n-gram, bad words) — by loops
// over the prefix and the bad-word table that stride over the workgroup.  The log-softmax
// statistics are reduced from the registers before any edit; the edits are then applied where
// min-length drops eos: every thread tests the EPV bits of each vector it holds (two LDS words
// per bitmap and vector).  A forced token needs no selection at all: the row is reduced for
// the log-prob and the thread 0 writes the forced id, kept count 1, smallest kept logit 0.
//
// DEV: the device-clock step (instantiations of their own; DEV = false leaves the three kernels
// above as they were).  t, T and cur_len0 are loaded from the clock once at the top of the
// workgroup (uniform loads from a kernel-argument pointer).  A step with t outside
// [0, min(T of the buffers, T of the clock)) is dead: every thread leaves before any store, and
// no address is formed from t.  A live step sets the per-token fields the host entries receive
// by value — the record column, the suppressed eos, the forced token, the length of the prefix's
// second segment, this step's row of the uniforms — and runs the step unchanged.
template <class DT, int NV, int NT, bool REC = false, bool PROC = false, bool DEV = false>
__global__ __launch_bounds__(NT) void k_ppo_sample(ppo_sample_args_t<REC, PROC, DEV> args) {
    static_assert(REC || !PROC, "the processing step carries the record block");
    static_assert(REC || !DEV, "the device-clock step carries the record block");
    [[maybe_unused]] PpoSampleArgs a_clock;
    PpoRecordArgs r_step = record_args(args);
    [[maybe_unused]] PpoProcArgs p_step = proc_args(args);
    if constexpr (DEV) {
        const PpoClockArgs c = args.c;
        const int64_t tc = c.clock[TRLX_CLOCK_T], cap = c.clock[TRLX_CLOCK_CAP];
        const int64_t cur_len = c.clock[TRLX_CLOCK_CUR_LEN0] + tc;
        if (tc < 0 || tc >= (cap < c.T ? cap : c.T)) return;  // block-uniform, before any barrier
        a_clock = args.s;
        a_clock.suppress_eos = a_clock.eos >= 0 && cur_len < c.min_length;
        a_clock.u = a_clock.u + tc * c.u_ld;
        r_step.t = tc;
        if constexpr (PROC) {
            p_step.n1 = int(tc);
            p_step.forced = c.forced_eos >= 0 && cur_len == c.max_length - 1 ? c.forced_eos
                            : c.forced_bos >= 0 && cur_len == 1              ? c.forced_bos
                                                                             : -1;
        }
    }
    const PpoSampleArgs& a = DEV ? a_clock : sample_args(args);
    const PpoRecordArgs r = r_step;
    [[maybe_unused]] const PpoProcArgs p = p_step;
    [[maybe_unused]] bool rec_on = true;  // PROC: recording is a run-time choice (block-uniform)
    if constexpr (PROC) rec_on = r.ref_logits != nullptr;
    constexpr int kWaves = NT / kWave;
    typedef typename DT::elem_t E;
    constexpr int EPV = DT::kEPV;
    constexpr int NSEG = NV + 2;  // index-order segments: head elements, vector steps, tail
    static_assert(kPsCandCap <= NT, "one candidate per thread");
    __shared__ float sh_red[kWaves];
    __shared__ double sh_sum[kWaves];
    __shared__ float sh_red3[kWaves];
    __shared__ int cnt[2][kWaves];           // bisection counts / masses (double-buffered)
    __shared__ float mass[2][kWaves];
    __shared__ float seg_tot[NSEG][kWaves];
    __shared__ float seg_pre[NSEG + 1];
    __shared__ int s_pick[3];                // segment, winning thread, token
    __shared__ float s_rem, s_lp;
    __shared__ int w_cnt[kWaves];            // kept count / smallest kept logit per wave
    __shared__ float w_min[kWaves];
    __shared__ float t_max[NT];              // per-thread maximum
    __shared__ __align__(16) float c_val[kPsCandCap + 4];  // candidates: every x >= t0
    __shared__ __align__(16) float c_w[kPsCandCap + 4];    // their weights
    __shared__ int c_n, s_bad;
    __shared__ uint32_t s_minkey;
    __shared__ float s_thr;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x;
    const int64_t V = a.V;
    const int64_t padtok = a.pad < 0 ? 0 : a.pad;
    auto finish = [&](int64_t tok, float lp, float mn, int n) {  // one thread
        a.out_ids[b] = tok;
        a.out_lp[b] = lp;
        a.out_min[b] = mn;
        a.out_cnt[b] = n;
    };
    // column t of the rollout's buffers (one thread); scored: the row was read, else 0 / 0 / 0
    auto record = [&](int64_t tok, float lp, float rlp, bool scored, bool live) __attribute__((always_inline)) {
        r.tokens[b * r.ld_tokens + r.t] = tok;
        r.lp[b * r.ld_lp + r.t] = lp;
        r.ref_lp[b * r.ld_ref_lp + r.t] = rlp;
        if (r.values) r.values[b * r.ld_values + r.t] = scored ? ld_any(r.v, r.v_dtype, b) : 0.f;
        if (live && r.lengths && a.eos >= 0 && tok == a.eos) r.lengths[b] = r.t + 1;
    };
    [[maybe_unused]] bool pad_scored = false;  // the recording step's finished row that still scores pad
    if constexpr (REC) {
        const bool finished = a.unfinished && a.unfinished[b] == 0;
        pad_scored = finished && r.score_finished;
        if constexpr (PROC) pad_scored = pad_scored && rec_on;
        if (finished && !pad_scored) {  // pad, 0, 0; neither row is read
            if (tid == 0) {
                finish(padtok, 0.f, 0.f, 0);
                if (rec_on) record(padtok, 0.f, 0.f, false, false);
            }
            return;
        }
    } else if (a.unfinished && a.unfinished[b] == 0) {  // a finished row emits pad and stays finished
        if (tid == 0) finish(padtok, 0.f, 0.f, 0);
        return;
    }

    // ---- processing step: the edit bitmaps.  Bit v of `pen` / `ban`: token v takes the
    // repetition penalty / becomes -inf.  A prefix token outside [0, V) sets no bit (tested
    // before any address is formed) but keeps its position in the n-gram and bad-word matches,
    // where the comparison is on the int64 values.  One spare word: a vector's bits are read
    // as the two words from its first element's.  (V < NV * NT * EPV by the launch table.)
    constexpr int kBmWords = PROC ? NV * NT * DT::kEPV / 32 + 2 : 1;
    __shared__ uint32_t pen[kBmWords], ban[kBmWords];
    if constexpr (PROC) {
        if (p.edits && p.forced < 0) {  // block-uniform
            const int nw = int((V + 31) / 32) + 1;
            for (int i = tid; i < nw; i += NT) {
                pen[i] = 0u;
                ban[i] = 0u;
            }
            __syncthreads();
            const int n = p.n0 + p.n1;
            auto ptok = [&](int j) __attribute__((always_inline)) {
                return j < p.n0 ? p.seg0[b * p.ld0 + j] : p.seg1[b * p.ld1 + (j - p.n0)];
            };
            auto mark = [&](uint32_t* bm, int64_t tok) __attribute__((always_inline)) {
                if (uint64_t(tok) < uint64_t(V)) atomicOr(&bm[int(tok >> 5)], 1u << int(tok & 31));
            };
            if (p.rp != 1.f)
                for (int j = tid; j < n; j += NT) mark(pen, ptok(j));
            const int g = p.ngram;
            if (g > 0 && n + 1 >= g) {  // p[i : i + g - 1] == p[n - g + 1 : n] bans p[i + g - 1]
                for (int i = tid; i + g - 1 < n; i += NT) {
                    bool eq = true;
                    for (int q = 0; eq && q < g - 1; ++q) eq = ptok(i + q) == ptok(n - g + 1 + q);
                    if (eq) mark(ban, ptok(i + g - 1));
                }
            }
            for (int sq = tid; sq < p.n_bw; sq += NT) {  // [w0 .. wk] bans wk after a prefix ending w0 .. w(k-1)
                const int64_t o = p.bw_off[sq];
                const int k = int(p.bw_off[sq + 1] - o) - 1;
                if (k < 0 || k > n) continue;
                bool eq = true;
                for (int q = 0; eq && q < k; ++q) eq = ptok(n - k + q) == p.bw_tok[o + q];
                if (eq) mark(ban, p.bw_tok[o + k]);
            }
            // (read after the barrier that the policy row's statistics take below)
        }
    }

    // ---- recording step: the reference row, streamed once on its own head / body / tail split
    // and line shift: per-thread online (max, sum exp) in fp32 over the steps in order, then the
    // wave's pair in LDS.  The pairs are combined in wave order by ref_logprob(), after the
    // barrier that the policy row's statistics take below.
    __shared__ float r_max[REC ? kWaves : 1], r_sum[REC ? kWaves : 1], s_rlp;
    const E* xr = nullptr;
    if constexpr (REC) if (rec_on) {
        xr = reinterpret_cast<const E*>(r.ref_logits) + b * r.ld_ref;
        const RowSplit<DT> sr(xr, V);
        const int nvr = int(sr.nvec);
        const int shr = line_shift(xr + sr.head);
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(xr + sr.head, uint32_t(nvr) * 16u);
        vec4u raw[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k)
            raw[k] = __builtin_amdgcn_raw_buffer_load_b128(rr, (tid - shr) * 16 + k * NT * 16, 0, kAuxNT);
        int64_t jr = -1;
        if (tid < sr.head) jr = tid;
        else if (tid >= NT - sr.tail) jr = sr.tail0 + (tid - (NT - sr.tail));
        float rm = jr >= 0 ? DT::load1(xr, jr) : -INFINITY;
        float rs = rm == -INFINITY ? 0.f : 1.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            if (unsigned(tid - shr + k * NT) >= unsigned(nvr)) continue;  // outside the row: reads 0
            float g[EPV];
            DT::unpack(raw[k], g);
            float vm = g[0];
#pragma unroll
            for (int e = 1; e < EPV; ++e) vm = fmaxf(vm, g[e]);
            if (vm > rm) {  // rescale what is summed so far (0 while rm = -inf)
                rs *= exp2_fast((rm - vm) * kLog2e);
                rm = vm;
            }
            if (rm != -INFINITY) {
#pragma unroll
                for (int e = 0; e < EPV; ++e) rs += exp2_fast((g[e] - rm) * kLog2e);
            }
        }
        const float wm = wave_max(rm);
        rs = rm == -INFINITY ? 0.f : rs * exp2_fast((rm - wm) * kLog2e);
        rs = wave_sum(rs);
        if (lane == 0) {
            r_max[wv] = wm;
            r_sum[wv] = rs;
        }
    }
    // log_softmax(x_ref)[tok] (one thread, after a barrier): the difference first, as for the policy row
    auto ref_logprob = [&](int64_t tok) __attribute__((always_inline)) {
        float m = r_max[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) m = fmaxf(m, r_max[w]);
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w)
            if (r_max[w] != -INFINITY) sum += r_sum[w] * exp2_fast((r_max[w] - m) * kLog2e);
        return (DT::load1(xr, tok) - m) - logf(sum);
    };

    const E* x = reinterpret_cast<const E*>(a.logits) + b * a.ld_logits;
    const RowSplit<DT> s(x, V);
    const int nvec = int(s.nvec);
    const int shift = line_shift(x + s.head);
    const int voff = (tid - shift) * 16;
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(x + s.head, uint32_t(nvec) * 16u);
    auto valid = [&](int k) { return unsigned(tid - shift + k * NT) < unsigned(nvec); };
    // recomputed at every use (laundered): CSE would keep NV 64-bit indices live across the kernel
    auto index_of = [&](int k, int e) {
        return s.head + int64_t(launder_int(tid - shift) + k * NT) * EPV + e;
    };

    // ---- logits row -> registers (out-of-row entries -inf); <= 1 edge element per thread
    float f[NV][EPV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const vec4u v = __builtin_amdgcn_raw_buffer_load_b128(rin, launder_int(voff) + k * NT * 16, 0, kAuxNT);
        DT::unpack(v, f[k]);
    }
    int64_t je = -1;  // head element -> threads [0, head); tail -> the last `tail` threads
    if (tid < s.head) je = tid;
    else if (tid >= NT - s.tail) je = s.tail0 + (tid - (NT - s.tail));
    float fe = je >= 0 ? DT::load1(x, je) : -INFINITY;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int e = 0; e < EPV; ++e)
            if (!valid(k)) f[k][e] = -INFINITY;

    // ---- log_softmax statistics of the unmodified row: exponentials relative to the wave
    // maximum, then one exchange of (wave max, wave sum) pairs — one barrier
    float m = fe;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int e = 0; e < EPV; ++e) m = fmaxf(m, f[k][e]);
    m = wave_max(m);
    const float mo = m == -INFINITY ? 0.f : m * kLog2e;
    // (summed in fp64: when one token holds nearly all the mass the sum is 1 + a small rest,
    // and the rest is the token's log-prob — fp32 partial sums would round it away)
    double sum = exp2_fast(__builtin_fmaf(fe, kLog2e, -mo));
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int e = 0; e < EPV; ++e) sum += double(exp2_fast(__builtin_fmaf(f[k][e], kLog2e, -mo)));
        __builtin_amdgcn_sched_barrier(0);  // one step's exponentials in flight, not the row's
    }
    sum = wave_sum_d(sum);
    if (lane == 0) {
        // mo is rounded, so every term above carries the factor 2^(m * log2e - mo) (off 1 by
        // up to 7e-7), the maximum's own term included — and that one must count as exactly 1
        // for log(sum) to keep the small rest.  d is that term bit for bit: divide it out
        // (1 / d = 1 - e + e^2 to fp64 for e = d - 1)
        const double e = double(exp2_fast(__builtin_fmaf(m, kLog2e, -mo))) - 1.0;
        sh_red[wv] = m;
        sh_sum[wv] = sum * (1.0 - e + e * e);
    }
    __syncthreads();
    m = sh_red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = fmaxf(m, sh_red[w]);
    sum = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (sh_red[w] != -INFINITY) sum += sh_sum[w] * double(exp2_fast((sh_red[w] - m) * kLog2e));
    // log_softmax(x)[j] = (x_j - m) - log(sum): the difference first, so a token that holds
    // nearly all the mass keeps a log-prob near 0 to fp32 relative precision
    const float row_max = m, log_sum = float(log(sum));
    if constexpr (REC) {
        if (pad_scored) {  // block-uniform: no selection, no draw, the row stays finished
            if (tid == 0) {
                const float lp = (DT::load1(x, padtok) - row_max) - log_sum;
                finish(padtok, lp, 0.f, 0);
                record(padtok, lp, ref_logprob(padtok), true, false);
            }
            return;
        }
    }
    if constexpr (PROC) {
        // ---- forced token: every other entry is -inf and this one 0 — nothing to select or draw
        if (p.forced >= 0) {  // block-uniform
            if (tid == 0) {
                const int64_t tok = p.forced;
                const float lp = (DT::load1(x, tok) - row_max) - log_sum;
                finish(tok, lp, 0.f, 1);
                if (rec_on) record(tok, lp, ref_logprob(tok), true, true);
                if (a.unfinished && a.eos >= 0) a.unfinished[b] = tok != a.eos ? 1 : 0;
            }
            return;
        }
    }

    // ---- min length: the thread that holds x[eos] drops it; the row maximum again
    float xmax = m;
    if constexpr (PROC) {
        // ---- the processors' edits, in HF's order: repetition penalty (fp32, a true
        // multiplication / division), then the bans; min length follows as in the plain step
        if (p.edits) {  // block-uniform
            const float rp = p.rp;
            auto edit = [&](float v, bool pn, bool bn) __attribute__((always_inline)) {
                if (pn) v = v < 0.f ? __fmul_rn(v, rp) : __fdiv_rn(v, rp);
                return bn ? -INFINITY : v;
            };
            if (je >= 0) fe = edit(fe, (pen[je >> 5] >> (je & 31)) & 1u, (ban[je >> 5] >> (je & 31)) & 1u);
            float mx = fe;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                if (valid(k)) {
                    const int64_t j0 = index_of(k, 0);
                    const int w = int(j0 >> 5), sh = int(j0 & 31);
                    constexpr uint32_t kMask = (1u << EPV) - 1u;
                    const uint32_t pb = uint32_t(((uint64_t(pen[w + 1]) << 32 | pen[w]) >> sh)) & kMask;
                    const uint32_t bb = uint32_t(((uint64_t(ban[w + 1]) << 32 | ban[w]) >> sh)) & kMask;
                    if (pb | bb) {
#pragma unroll
                        for (int e = 0; e < EPV; ++e) f[k][e] = edit(f[k][e], (pb >> e) & 1u, (bb >> e) & 1u);
                    }
                }
#pragma unroll
                for (int e = 0; e < EPV; ++e) mx = fmaxf(mx, f[k][e]);
            }
            if (!a.suppress_eos) xmax = block_max(mx, sh_red3);
        }
    }
    if (a.suppress_eos) {  // block-uniform
        if (je == a.eos) fe = -INFINITY;
        int ks = -1, es = -1;
        if (a.eos >= s.head && a.eos < s.tail0) {
            const int64_t q = a.eos - s.head;
            const int slot = int(q / EPV) + shift;  // vector i sits in thread (i + shift) % NT, step (i + shift) / NT
            if (slot % NT == tid) {
                ks = slot / NT;
                es = int(q % EPV);
            }
        }
        float mx = fe;
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                if (k == ks && e == es) f[k][e] = -INFINITY;
                mx = fmaxf(mx, f[k][e]);
            }
        xmax = block_max(mx, sh_red3);
    }
    if (xmax == -INFINITY) {  // no finite logit left (HF's multinomial would raise): pad, nothing kept
        if (tid == 0) {
            finish(padtok, 0.f, 0.f, 0);
            if constexpr (REC) if (rec_on) record(padtok, 0.f, 0.f, true, true);
            if (a.unfinished && a.eos >= 0) a.unfinished[b] = padtok != a.eos ? 1 : 0;
        }
        return;
    }

    // (from here on a slot outside the row or suppressed holds -inf, which no count or
    // weight below can pick: no per-slot validity test is needed)
    const float scale = a.scale;
    auto weight_at = [&](float v, float xm) { return exp2_fast((v - xm) * scale); };  // exp((x - max) / T); 0 for -inf
    auto weight = [&](float v) { return weight_at(v, xmax); };
    // block-wide #(x >= cf) and mass{x >= lo}: per-thread partial, wave reduction, one LDS
    // exchange summed in wave order by every thread (double-buffered: one barrier per call)
    int par = 0;
    auto count_ge = [&](float cf) {
        int c = fe >= cf ? 1 : 0;
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int e = 0; e < EPV; ++e) c += f[k][e] >= cf ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
        if (lane == 0) cnt[par][wv] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) tot += cnt[par][w];
        par ^= 1;
        return tot;
    };
    auto mass_ge = [&](float lo) {
        // (laundered maximum: inside a bisection loop the weights are loop-invariant, and
        // hoisting them would hold the row twice in VGPRs)
        float xm = xmax;
        asm volatile("" : "+v"(xm));
        float t = fe >= lo ? weight_at(fe, xm) : 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
#pragma unroll
            for (int e = 0; e < EPV; ++e) t += f[k][e] >= lo ? weight_at(f[k][e], xm) : 0.f;
            __builtin_amdgcn_sched_barrier(0);  // one step's exponentials in flight, not the row's
        }
        t = wave_sum(t);
        if (lane == 0) mass[par][wv] = t;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) tot += mass[par][w];
        par ^= 1;
        return tot;
    };
    // the n-th largest x: bisection on the keys, MSB first — the largest key K with
    // #(key >= K) >= n IS the n-th largest key.  The candidate is turned into a float, not
    // every x into a key; float >= is monotone in the key, and candidates in the NaN key
    // ranges (skipped) would count 0.  Fewer than n finite values: -inf, all of them kept.
    auto nth_largest = [&](int n) __attribute__((always_inline)) {
        uint32_t K = 0;
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = K | (1u << bit);
            const float cf = fkey_inv(cand);
            if (cf != cf) continue;
            if (count_ge(cf) >= n) K = cand;
        }
        return K > fkey(-INFINITY) ? fkey_inv(K) : -INFINITY;
    };

    const int top_k = a.top_k;
    const bool nucleus = a.top_p < 1.f;
    float thr = -INFINITY;  // keep x >= thr (and finite)
    bool done = !(top_k > 0 && int64_t(top_k) < V) && !nucleus;  // nothing to filter
    float w_all = 0.f;
    if (!done && top_k == 0) w_all = mass_ge(-INFINITY);  // top-p alone: W over the whole row

    // ---- candidate list.  t0 = the n-th largest of the per-thread maxima is a lower bound of
    // the n-th largest x (n threads each own an x >= t0), so the values >= t0 — a few times n
    // on real rows — hold the n largest.  With top-k (n = k) that is every survivor, and the
    // nucleus is a subset of them.  With top-p alone (n = a seed) the list is an upper set
    // of the row: the mass above a candidate is exact, and the nucleus lies inside the list
    // iff the list's smallest value is not kept; otherwise the block-wide search runs.
    int n0 = top_k > 0 ? top_k : (kPsSeed > a.min_keep ? kPsSeed : a.min_keep);
    if (!done && n0 <= NT && int64_t(n0) < V) {
        float mx = fe;
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int e = 0; e < EPV; ++e) mx = fmaxf(mx, f[k][e]);
        t_max[tid] = mx;
        if (tid == 0) {
            c_n = 0;
            s_bad = 0;
            s_minkey = 0xffffffffu;
        }
        __syncthreads();
        if (wv == 0) {
            constexpr int R = NT / kWave;
            float tv[R];
#pragma unroll
            for (int i = 0; i < R; ++i) tv[i] = t_max[lane + i * kWave];
            // the top 16 key bits (sign, exponent, 7 mantissa bits) are enough for a lower
            // bound: K <= the exact key, a few more candidates at most
            uint32_t K = 0;
            for (int bit = 31; bit >= 16; --bit) {
                const uint32_t cand = K | (1u << bit);
                const float cf = fkey_inv(cand);
                int c = 0;
#pragma unroll
                for (int i = 0; i < R; ++i) c += __popcll(__ballot(tv[i] >= cf));
                if (c >= n0) K = cand;
            }
            if (lane == 0) s_thr = K > fkey(-INFINITY) ? fkey_inv(K) : -INFINITY;
        }
        __syncthreads();
        const float t0 = s_thr;
        if (t0 != -INFINITY) {
            auto append = [&](bool p, float v) {
                const uint64_t mk = __ballot(p);
                if (mk == 0) return;
                const int leader = __ffsll((unsigned long long)mk) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&c_n, __popcll(mk));
                base = __shfl(base, leader, kWave);
                const int pos = base + __builtin_amdgcn_mbcnt_hi(uint32_t(mk >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo(uint32_t(mk), 0));
                if (p && pos < kPsCandCap) c_val[pos] = v;
            };
            append(fe >= t0, fe);
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int e = 0; e < EPV; ++e) append(f[k][e] >= t0, f[k][e]);
        }
        __syncthreads();
        const int n = c_n;
        if (t0 != -INFINITY && n <= kPsCandCap) {  // block-uniform
            if (tid < 4) {  // pad to whole float4s: -inf and zero weights never count
                c_val[n + tid] = -INFINITY;
                c_w[n + tid] = 0.f;
            }
            __syncthreads();
            // every thread ranks at most one candidate against the whole list (LDS broadcast
            // reads): the k-th largest is the value with #(>) < k <= #(>=) — exact, with ties
            const bool own = tid < n;
            const float vt = own ? c_val[tid] : -INFINITY;
            int gt = 0, ge = 0;
            for (int q = 0; q < n; q += 4) {
                const float4 vq = *reinterpret_cast<const float4*>(&c_val[q]);
                gt += (vq.x > vt) + (vq.y > vt) + (vq.z > vt) + (vq.w > vt);
                ge += (vq.x >= vt) + (vq.y >= vt) + (vq.z >= vt) + (vq.w >= vt);
            }
            float thr_k = -INFINITY;
            if (top_k > 0) {
                if (own && gt < top_k && top_k <= ge) s_thr = vt;  // every writer holds the same value
                __syncthreads();
                thr_k = s_thr;
            }
            const bool surv = own && vt >= thr_k;
            if (own) c_w[tid] = surv ? weight(vt) : 0.f;
            __syncthreads();
            bool kept = surv;
            if (nucleus) {
                float above = 0.f, tot = 0.f;  // mass of the survivors strictly above vt; all survivors
                for (int q = 0; q < n; q += 4) {
                    const float4 vq = *reinterpret_cast<const float4*>(&c_val[q]);
                    const float4 wq = *reinterpret_cast<const float4*>(&c_w[q]);
                    tot += wq.x + wq.y + wq.z + wq.w;
                    above += (vq.x > vt ? wq.x : 0.f) + (vq.y > vt ? wq.y : 0.f) + (vq.z > vt ? wq.z : 0.f) +
                             (vq.w > vt ? wq.w : 0.f);
                }
                const float W = top_k > 0 ? tot : w_all;
                kept = surv && (above <= a.top_p * W || gt < a.min_keep);
                if (top_k == 0 && kept && ge == n) s_bad = 1;  // the list's smallest value is kept
            }
            if (kept) atomicMin(&s_minkey, fkey(vt));
            __syncthreads();
            if (!s_bad) {
                thr = fkey_inv(s_minkey);
                done = true;
            }
        }
    }
    if (!done) {
        // ---- block-wide searches over the whole row
        const float thr_k = (top_k > 0 && int64_t(top_k) < V) ? nth_largest(top_k) : -INFINITY;
        thr = thr_k;
        if (nucleus) {
            // the smallest row value whose strictly-greater mass is <= top_p * W is the
            // largest key K with mass{key >= K} > top_p * W (mass{key >= K + 1} is then
            // <= top_p * W, so K itself carries mass: it is a row value)
            const float pw = a.top_p * (top_k == 0 ? w_all : mass_ge(thr_k));
            uint32_t K = 0;
#pragma unroll 1
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = K | (1u << bit);
                const float cf = fkey_inv(cand);
                if (cf != cf) continue;
                if (mass_ge(fmaxf(cf, thr_k)) > pw) K = cand;
            }
            float thr_p = K > fkey(-INFINITY) ? fkey_inv(K) : -INFINITY;
            if (a.min_keep > 1) thr_p = fminf(thr_p, nth_largest(a.min_keep));
            thr = fmaxf(thr_p, thr_k);
        }
    }

    // ---- weights of the kept entries, their count and smallest value
    auto kept = [&](float v) { return v >= thr && v != -INFINITY; };
    const float ew = kept(fe) ? weight(fe) : 0.f;
    const int eseg = je < s.head ? 0 : NSEG - 1;  // the edge element's segment
    int nk = kept(fe) ? 1 : 0;
    float mn = kept(fe) ? fe : INFINITY;
    // the registers now hold the unnormalised probabilities; per-wave segment totals go
    // straight to LDS (no per-thread segment array: it would spill at 1024 threads)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float t = 0.f;
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
            const bool kp = kept(f[k][e]);
            nk += kp ? 1 : 0;
            mn = kp ? fminf(mn, f[k][e]) : mn;
            const float w = kp ? weight(f[k][e]) : 0.f;
            f[k][e] = w;
            t += w;
        }
        t = wave_sum(t);
        if (lane == 0) seg_tot[1 + k][wv] = t;
        __builtin_amdgcn_sched_barrier(0);
    }
    {
        const float t0 = wave_sum(eseg == 0 ? ew : 0.f), t1 = wave_sum(eseg == 0 ? 0.f : ew);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nk += __shfl_xor(nk, off, kWave);
        mn = -wave_max(-mn);
        if (lane == 0) {
            seg_tot[0][wv] = t0;
            seg_tot[NSEG - 1][wv] = t1;
            w_cnt[wv] = nk;
            w_min[wv] = mn;
        }
    }

    // ---- inverse CDF at u: segment totals (fixed order) -> segment -> thread -> element
    __syncthreads();
    if (tid == 0) {
        float acc = 0.f;
        for (int g = 0; g < NSEG; ++g) {
            seg_pre[g] = acc;
            for (int w = 0; w < kWaves; ++w) acc += seg_tot[g][w];
        }
        seg_pre[NSEG] = acc;
        const float target = a.u[b] * acc;
        int gsel = -1;
        for (int g = 0; g < NSEG; ++g)
            if (gsel < 0 && seg_pre[g + 1] > target) gsel = g;
        for (int g = NSEG - 1; gsel < 0 && g >= 0; --g)  // rounding at the top: last non-empty
            if (seg_pre[g + 1] > seg_pre[g]) gsel = g;
        s_pick[0] = gsel;
        s_pick[1] = -1;
        s_pick[2] = -1;
        s_lp = 0.f;
        s_rem = gsel < 0 ? 0.f : target - seg_pre[gsel];
    }
    __syncthreads();
    const int gsel = s_pick[0];
    const float rem = s_rem;
    float mine = 0.f, lo = 0.f;
    if (gsel >= 0) {
        if (gsel == 0 || gsel == NSEG - 1) {
            mine = (je >= 0 && eseg == gsel) ? ew : 0.f;
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                // (opaque zero: the same sums exist in the pass above, and reusing them would
                // keep NV more registers live across it)
                float t = 0.f;
                asm volatile("" : "+v"(t));
#pragma unroll
                for (int e = 0; e < EPV; ++e) t += f[k][e];
                mine = k + 1 == gsel ? t : mine;
            }
        }
        float incl = mine;  // exclusive prefix of this thread's share inside the segment
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const float y = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += y;
        }
        float woff = 0.f;
        for (int w = 0; w < wv; ++w) woff += seg_tot[gsel][w];
        lo = woff + incl - mine;
        // the last thread (index order) whose share starts at or below the target
        if (mine > 0.f && lo <= rem) atomicMax(&s_pick[1], tid);
    }
    __syncthreads();
    if (gsel >= 0 && tid == s_pick[1]) {
        int64_t pick = -1;
        if (gsel == 0 || gsel == NSEG - 1) {
            pick = je;
        } else {
            float run = lo;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                if (k + 1 != gsel) continue;
#pragma unroll
                for (int e = 0; e < EPV; ++e) {
                    if (f[k][e] > 0.f && (pick < 0 || run <= rem)) {
                        pick = index_of(k, e);
                        run += f[k][e];
                        if (run > rem) run = INFINITY;  // found: later elements keep the pick
                    }
                }
            }
        }
        s_pick[2] = int(pick);
        // the row's registers hold weights by now: the drawn logit comes from memory again
        if (pick >= 0) s_lp = (DT::load1(x, pick) - row_max) - log_sum;
        if constexpr (REC) if (rec_on) s_rlp = pick >= 0 ? ref_logprob(pick) : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        float mnk = INFINITY;
        for (int w = 0; w < kWaves; ++w) {
            n += w_cnt[w];
            mnk = fminf(mnk, w_min[w]);
        }
        const bool got = s_pick[2] >= 0;
        const int64_t tok = got ? s_pick[2] : padtok;
        finish(tok, got ? s_lp : 0.f, got ? mnk : 0.f, got ? n : 0);
        if constexpr (REC) if (rec_on) record(tok, got ? s_lp : 0.f, got ? s_rlp : 0.f, true, true);
        if (a.unfinished && a.eos >= 0) a.unfinished[b] = tok != a.eos ? 1 : 0;
    }
}

}  // namespace trlx

using namespace trlx;

// All entries: the arguments they share, one launch table.  rec = NULL: the plain step;
// proc = NULL: the kernels without the processing step.
static int ppo_sample_launch(const char* who, const void* logits, int64_t ld_logits, int dtype, int64_t B, int64_t V,
                             float temperature, int top_k, float top_p, int min_tokens_to_keep, int64_t cur_len,
                             int64_t min_length, int64_t eos_token_id, int64_t pad_token_id, const float* u,
                             int64_t* out_ids, float* out_logprobs, float* out_min_kept, int32_t* out_kept_count,
                             int64_t* unfinished, const PpoRecordArgs* rec, void* stream,
                             const PpoProcArgs* proc = nullptr, const PpoClockArgs* clk = nullptr) {
    TRLX_REQUIRE(B == 0 || (logits && u && out_ids && out_logprobs && out_min_kept && out_kept_count), TRLX_ERR_ARG,
                 "NULL argument to %s", who);
    TRLX_REQUIRE(dtype == TRLX_F32 || dtype == TRLX_BF16, TRLX_ERR_DTYPE, "dtype %d", dtype);
    TRLX_REQUIRE(B >= 0 && V > 0, TRLX_ERR_SHAPE, "bad shape");
    TRLX_REQUIRE(temperature > 0.f && top_p > 0.f && top_k >= 0 && min_tokens_to_keep >= 1, TRLX_ERR_ARG,
                 "bad sampling arguments (temperature > 0, top_p > 0, top_k >= 0, min_tokens_to_keep >= 1)");
    TRLX_REQUIRE(eos_token_id >= -1 && eos_token_id < V && pad_token_id >= -1 && pad_token_id < V, TRLX_ERR_ARG,
                 "eos / pad token outside [0, V) (-1 = none)");
    TRLX_REQUIRE(B < (int64_t(1) << 31) && V * 16 < (int64_t(1) << 32), TRLX_ERR_SHAPE, "too large");
    if (B == 0) return TRLX_OK;
    PpoSampleArgs a = {};
    a.logits = logits;
    a.ld_logits = ld_logits;
    a.V = V;
    a.scale = kLog2e / temperature;
    a.top_p = top_p;
    a.min_keep = int(min_tokens_to_keep < V ? min_tokens_to_keep : V);
    a.top_k = top_k == 0 ? 0 : int(top_k < a.min_keep ? a.min_keep : (top_k < V ? top_k : V));
    a.suppress_eos = eos_token_id >= 0 && cur_len < min_length;
    a.eos = eos_token_id;
    a.pad = pad_token_id;
    a.u = u;
    a.out_ids = out_ids;
    a.out_lp = out_logprobs;
    a.out_min = out_min_kept;
    a.out_cnt = out_kept_count;
    a.unfinished = unfinished;
    const int epv = dtype == TRLX_BF16 ? 8 : 4;
    auto need = [&](int nt) { return (V / epv + 1 + (kLineVecs - 1) + nt - 1) / nt; };  // vectors per thread
    // (the table of trlx_ilql_sample without its 128-VGPR rows — 16 x 8 bf16, 32 x 4 fp32 — which
    // cannot hold the row beside this kernel's state without scratch: rows end at ~53k entries)
#define TRLX_PSMP(DTT, N, NT)                                                                                  \
    if (need(NT) <= N) {                                                                                       \
        if (clk && proc) {                                                                                     \
            hipLaunchKernelGGL((k_ppo_sample<DTT, N, NT, true, true, true>), dim3(unsigned(B)), dim3(NT), 0,   \
                               (hipStream_t)stream, PpoSampleProcClockArgs{a, *rec, *proc, *clk});             \
            return check_launch("k_ppo_sample<proc, clock>");                                                  \
        }                                                                                                      \
        if (clk) {                                                                                             \
            hipLaunchKernelGGL((k_ppo_sample<DTT, N, NT, true, false, true>), dim3(unsigned(B)), dim3(NT), 0,  \
                               (hipStream_t)stream, PpoSampleRecClockArgs{a, *rec, *clk});                     \
            return check_launch("k_ppo_sample<record, clock>");                                                \
        }                                                                                                      \
        if (proc) {                                                                                            \
            hipLaunchKernelGGL((k_ppo_sample<DTT, N, NT, true, true>), dim3(unsigned(B)), dim3(NT), 0,         \
                               (hipStream_t)stream, PpoSampleProcArgs{a, rec ? *rec : PpoRecordArgs{}, *proc}); \
            return check_launch("k_ppo_sample<proc>");                                                         \
        }                                                                                                      \
        if (rec) {                                                                                             \
            hipLaunchKernelGGL((k_ppo_sample<DTT, N, NT, true>), dim3(unsigned(B)), dim3(NT), 0,               \
                               (hipStream_t)stream, PpoSampleRecArgs{a, *rec});                                \
            return check_launch("k_ppo_sample<record>");                                                       \
        }                                                                                                      \
        hipLaunchKernelGGL((k_ppo_sample<DTT, N, NT>), dim3(unsigned(B)), dim3(NT), 0, (hipStream_t)stream, a); \
        return check_launch("k_ppo_sample");                                                                   \
    }
    if (dtype == TRLX_BF16) {
        TRLX_PSMP(BF16T, 1, 1024)
        TRLX_PSMP(BF16T, 4, 1024)
        TRLX_PSMP(BF16T, 8, 512)
        TRLX_PSMP(BF16T, 13, 512)
    } else {
        TRLX_PSMP(F32T, 1, 1024)
        TRLX_PSMP(F32T, 4, 1024)
        TRLX_PSMP(F32T, 8, 1024)
        TRLX_PSMP(F32T, 16, 512)
        TRLX_PSMP(F32T, 26, 512)
    }
#undef TRLX_PSMP
    TRLX_REQUIRE(false, TRLX_ERR_SHAPE, "vocab %lld too long for the sampling kernel", (long long)V);
}

extern "C" int trlx_ppo_sample(const void* logits, int64_t ld_logits, int dtype, int64_t B, int64_t V,
                               float temperature, int top_k, float top_p, int min_tokens_to_keep,
                               int64_t cur_len, int64_t min_length, int64_t eos_token_id, int64_t pad_token_id,
                               const float* u, int64_t* out_ids, float* out_logprobs, float* out_min_kept,
                               int32_t* out_kept_count, int64_t* unfinished, void* stream) {
    return ppo_sample_launch("trlx_ppo_sample", logits, ld_logits, dtype, B, V, temperature, top_k, top_p,
                             min_tokens_to_keep, cur_len, min_length, eos_token_id, pad_token_id, u, out_ids,
                             out_logprobs, out_min_kept, out_kept_count, unfinished, nullptr, stream);
}

// The recording entries: the record block's checks, then the launch (proc = NULL: trlx_ppo_sample_record).
static int ppo_sample_record_launch(const char* who, const void* logits, int64_t ld_logits, int dtype, int64_t B,
                                    int64_t V, float temperature, int top_k, float top_p, int min_tokens_to_keep,
                                    int64_t cur_len, int64_t min_length, int64_t eos_token_id, int64_t pad_token_id,
                                    const float* u, int64_t* out_ids, float* out_logprobs, float* out_min_kept,
                                    int32_t* out_kept_count, int64_t* unfinished, const void* ref_logits,
                                    int64_t ld_ref, int ref_dtype, int64_t t, int64_t T, int64_t* tokens,
                                    int64_t ld_tokens, float* logprobs, int64_t ld_logprobs, float* ref_logprobs,
                                    int64_t ld_ref_logprobs, float* values, int64_t ld_values,
                                    const void* step_values, int values_dtype, int64_t* lengths, int score_finished,
                                    void* stream, const PpoProcArgs* proc, const PpoClockArgs* clk = nullptr) {
    TRLX_REQUIRE(B == 0 || (ref_logits && tokens && logprobs && ref_logprobs), TRLX_ERR_ARG,
                 "NULL argument to %s (ref_logits, tokens, logprobs, ref_logprobs)", who);
    TRLX_REQUIRE(ref_dtype == dtype, TRLX_ERR_DTYPE, "reference rows of dtype %d, policy rows of dtype %d", ref_dtype,
                 dtype);
    TRLX_REQUIRE(T > 0 && (clk || (t >= 0 && t < T)), TRLX_ERR_SHAPE, "column t = %lld outside [0, T = %lld)", (long long)t,
                 (long long)T);
    TRLX_REQUIRE(ld_tokens >= T && ld_logprobs >= T && ld_ref_logprobs >= T && (!values || ld_values >= T),
                 TRLX_ERR_SHAPE, "a record buffer's row stride is below T = %lld", (long long)T);
    TRLX_REQUIRE(B <= 1 || V <= 0 || (ld_logits >= V && ld_ref >= V), TRLX_ERR_SHAPE,
                 "row strides %lld / %lld below V = %lld", (long long)ld_logits, (long long)ld_ref, (long long)V);
    TRLX_REQUIRE((values == nullptr) == (step_values == nullptr), TRLX_ERR_ARG,
                 "values (the [B, T] buffer) and step_values (this step's [B]) go together");
    TRLX_REQUIRE(!values || values_dtype == TRLX_F32 || values_dtype == TRLX_BF16, TRLX_ERR_DTYPE,
                 "step_values dtype %d", values_dtype);
    PpoRecordArgs r = {};
    r.ref_logits = ref_logits;
    r.ld_ref = ld_ref;
    r.t = t;
    r.tokens = tokens;
    r.ld_tokens = ld_tokens;
    r.lp = logprobs;
    r.ld_lp = ld_logprobs;
    r.ref_lp = ref_logprobs;
    r.ld_ref_lp = ld_ref_logprobs;
    r.values = values;
    r.ld_values = ld_values;
    r.v = step_values;
    r.v_dtype = values_dtype;
    r.score_finished = score_finished != 0;
    r.lengths = lengths;
    return ppo_sample_launch(who, logits, ld_logits, dtype, B, V, temperature, top_k, top_p, min_tokens_to_keep,
                             cur_len, min_length, eos_token_id, pad_token_id, u, out_ids, out_logprobs, out_min_kept,
                             out_kept_count, unfinished, &r, stream, proc, clk);
}

extern "C" int trlx_ppo_sample_record(const void* logits, int64_t ld_logits, int dtype, int64_t B, int64_t V,
                                      float temperature, int top_k, float top_p, int min_tokens_to_keep,
                                      int64_t cur_len, int64_t min_length, int64_t eos_token_id,
                                      int64_t pad_token_id, const float* u, int64_t* out_ids, float* out_logprobs,
                                      float* out_min_kept, int32_t* out_kept_count, int64_t* unfinished,
                                      const void* ref_logits, int64_t ld_ref, int ref_dtype, int64_t t, int64_t T,
                                      int64_t* tokens, int64_t ld_tokens, float* logprobs, int64_t ld_logprobs,
                                      float* ref_logprobs, int64_t ld_ref_logprobs, float* values, int64_t ld_values,
                                      const void* step_values, int values_dtype, int64_t* lengths,
                                      int score_finished, void* stream) {
    return ppo_sample_record_launch("trlx_ppo_sample_record", logits, ld_logits, dtype, B, V, temperature, top_k,
                                    top_p, min_tokens_to_keep, cur_len, min_length, eos_token_id, pad_token_id, u,
                                    out_ids, out_logprobs, out_min_kept, out_kept_count, unfinished, ref_logits,
                                    ld_ref, ref_dtype, t, T, tokens, ld_tokens, logprobs, ld_logprobs, ref_logprobs,
                                    ld_ref_logprobs, values, ld_values, step_values, values_dtype, lengths,
                                    score_finished, stream, nullptr);
}

// trlx_ppo_sample_proc (d = NULL) and trlx_ppo_sample_proc_dev: with d, the per-token scalars of
// *a (t, cur_len, forced_token_id, prefix1_len) are not read; the kernel takes them from the clock.
static int ppo_sample_proc_entry(const char* who, const TrlxPpoSampleProcArgs* a, const TrlxPpoSampleDevArgs* d,
                                 void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "NULL argument to %s", who);
    const int64_t V = a->V;
    const bool dev = d != nullptr;
    // the prefix's second segment: with the clock its length is t < T, and the record's own tokens
    // unless the caller names another buffer
    const int64_t* prefix1 = a->prefix1;
    int64_t prefix1_ld = a->prefix1_ld, prefix1_len = a->prefix1_len;
    int64_t forced = a->forced_token_id;
    if (dev) {
        TRLX_REQUIRE(d->clock, TRLX_ERR_ARG, "%s: NULL clock", who);
        TRLX_REQUIRE((reinterpret_cast<uintptr_t>(d->clock) & 7u) == 0, TRLX_ERR_ARG,
                     "%s: the clock is not aligned to 8 bytes", who);
        TRLX_REQUIRE(a->ref_logits, TRLX_ERR_ARG, "%s: the record block is required (ref_logits is NULL)", who);
        TRLX_REQUIRE(d->u_ld == 0 || d->u_ld >= a->B, TRLX_ERR_ARG, "%s: u_ld %lld (0, or a table row of >= B = %lld)",
                     who, (long long)d->u_ld, (long long)a->B);
        TRLX_REQUIRE(d->forced_bos_token_id >= -1 && d->forced_bos_token_id < V && d->forced_eos_token_id >= -1 &&
                         d->forced_eos_token_id < V,
                     TRLX_ERR_ARG, "%s: forced bos / eos token %lld / %lld outside [0, V) (-1 = none)", who,
                     (long long)d->forced_bos_token_id, (long long)d->forced_eos_token_id);
        TRLX_REQUIRE(d->forced_eos_token_id < 0 || d->max_length >= 1, TRLX_ERR_ARG,
                     "%s: forced_eos_token_id needs max_length >= 1, got %lld", who, (long long)d->max_length);
        TRLX_REQUIRE(a->T >= 1 && a->T < (int64_t(1) << 30), TRLX_ERR_SHAPE, "%s: T %lld", who, (long long)a->T);
        if (!prefix1) {
            prefix1 = a->tokens;
            prefix1_ld = a->ld_tokens;
        }
        prefix1_len = a->T - 1;  // the longest the kernel reads; checked as such below
        forced = -1;
    }
    TRLX_REQUIRE(a->repetition_penalty > 0.f, TRLX_ERR_ARG, "repetition_penalty %g must be > 0",
                 double(a->repetition_penalty));
    TRLX_REQUIRE(a->no_repeat_ngram_size >= 0, TRLX_ERR_ARG, "no_repeat_ngram_size %d must be >= 0",
                 a->no_repeat_ngram_size);
    TRLX_REQUIRE(forced >= -1 && forced < V, TRLX_ERR_ARG, "forced token %lld outside [0, V) (-1 = none)",
                 (long long)forced);
    TRLX_REQUIRE(a->prefix0_len >= 0 && prefix1_len >= 0 && a->prefix0_len + prefix1_len < (int64_t(1) << 30),
                 TRLX_ERR_SHAPE, "prefix lengths %lld + %lld", (long long)a->prefix0_len, (long long)prefix1_len);
    TRLX_REQUIRE((a->prefix0_len == 0 || a->prefix0) && (prefix1_len == 0 || prefix1), TRLX_ERR_ARG,
                 "a prefix segment with n > 0 and a NULL pointer");
    TRLX_REQUIRE((a->prefix0_len == 0 || a->prefix0_ld >= a->prefix0_len) &&
                     (prefix1_len == 0 || prefix1_ld >= prefix1_len),
                 TRLX_ERR_SHAPE, "a prefix segment's row stride is below its length");
    const int64_t nbw = a->n_bad_words;
    TRLX_REQUIRE(nbw >= 0 && nbw < (int64_t(1) << 30), TRLX_ERR_SHAPE, "n_bad_words %lld", (long long)nbw);
    if (nbw > 0) {  // the host mirror of the table is what is checked; the kernel bounds-checks every ban again
        TRLX_REQUIRE(a->bad_words && a->bad_words_offsets && a->bad_words_host && a->bad_words_offsets_host,
                     TRLX_ERR_ARG, "bad words: the device table and its host mirror (tokens, offsets) are needed");
        const int64_t* off = a->bad_words_offsets_host;
        TRLX_REQUIRE(off[0] == 0, TRLX_ERR_ARG, "bad-word offsets must start at 0");
        for (int64_t s = 0; s < nbw; ++s)
            TRLX_REQUIRE(off[s + 1] > off[s], TRLX_ERR_ARG, "bad-word offsets not ascending at sequence %lld",
                         (long long)s);
        for (int64_t i = 0; i < off[nbw]; ++i)
            TRLX_REQUIRE(a->bad_words_host[i] >= 0 && a->bad_words_host[i] < V, TRLX_ERR_ARG,
                         "bad-word token %lld outside [0, V)", (long long)a->bad_words_host[i]);
    }
    PpoProcArgs p = {};
    p.seg0 = a->prefix0;
    p.ld0 = a->prefix0_ld;
    p.n0 = int(a->prefix0_len);
    p.seg1 = prefix1;
    p.ld1 = prefix1_ld;
    p.n1 = dev ? 0 : int(prefix1_len);
    p.bw_tok = a->bad_words;
    p.bw_off = a->bad_words_offsets;
    p.n_bw = int(nbw);
    p.ngram = a->no_repeat_ngram_size;
    p.rp = a->repetition_penalty;
    p.edits = p.rp != 1.f || p.ngram > 0 || p.n_bw > 0;
    p.forced = forced;
    if (dev) {
        // a processor or either forced id set: the processing kernel, else the recording kernel
        const bool processing = p.edits || d->forced_bos_token_id >= 0 || d->forced_eos_token_id >= 0;
        PpoClockArgs c = {};
        c.clock = d->clock;
        c.T = a->T;
        c.min_length = a->min_length;
        c.forced_bos = d->forced_bos_token_id;
        c.forced_eos = d->forced_eos_token_id;
        c.max_length = d->max_length;
        c.u_ld = d->u_ld;
        return ppo_sample_record_launch(who, a->logits, a->ld_logits, a->dtype, a->B, V, a->temperature, a->top_k,
                                        a->top_p, a->min_tokens_to_keep, 0, a->min_length, a->eos_token_id,
                                        a->pad_token_id, a->u, a->out_ids, a->out_logprobs, a->out_min_kept,
                                        a->out_kept_count, a->unfinished, a->ref_logits, a->ld_ref, a->ref_dtype, 0,
                                        a->T, a->tokens, a->ld_tokens, a->logprobs, a->ld_logprobs, a->ref_logprobs,
                                        a->ld_ref_logprobs, a->values, a->ld_values, a->step_values, a->values_dtype,
                                        a->lengths, a->score_finished, stream, processing ? &p : nullptr, &c);
    }
    // every processor off and no forced token: the kernels of the other two entries
    const PpoProcArgs* proc = (p.edits || p.forced >= 0) ? &p : nullptr;
    if (a->ref_logits)
        return ppo_sample_record_launch("trlx_ppo_sample_proc", a->logits, a->ld_logits, a->dtype, a->B, V,
                                        a->temperature, a->top_k, a->top_p, a->min_tokens_to_keep, a->cur_len,
                                        a->min_length, a->eos_token_id, a->pad_token_id, a->u, a->out_ids,
                                        a->out_logprobs, a->out_min_kept, a->out_kept_count, a->unfinished,
                                        a->ref_logits, a->ld_ref, a->ref_dtype, a->t, a->T, a->tokens, a->ld_tokens,
                                        a->logprobs, a->ld_logprobs, a->ref_logprobs, a->ld_ref_logprobs, a->values,
                                        a->ld_values, a->step_values, a->values_dtype, a->lengths,
                                        a->score_finished, stream, proc);
    return ppo_sample_launch("trlx_ppo_sample_proc", a->logits, a->ld_logits, a->dtype, a->B, V, a->temperature,
                             a->top_k, a->top_p, a->min_tokens_to_keep, a->cur_len, a->min_length, a->eos_token_id,
                             a->pad_token_id, a->u, a->out_ids, a->out_logprobs, a->out_min_kept, a->out_kept_count,
                             a->unfinished, nullptr, stream, proc);
}

extern "C" int trlx_ppo_sample_proc(const TrlxPpoSampleProcArgs* a, void* stream) {
    return ppo_sample_proc_entry("trlx_ppo_sample_proc", a, nullptr, stream);
}

extern "C" int trlx_ppo_sample_proc_dev(const TrlxPpoSampleProcArgs* a, const TrlxPpoSampleDevArgs* d, void* stream) {
    TRLX_REQUIRE(d, TRLX_ERR_ARG, "NULL device arguments to trlx_ppo_sample_proc_dev");
    return ppo_sample_proc_entry("trlx_ppo_sample_proc_dev", a, d, stream);
}
